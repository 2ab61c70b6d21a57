"""`quip_lib` operator boundary: same op names and schemas as the reference's
register_lib.py:8-192, implemented by the C-ABI library (capi.py) on the
caller's current HIP stream.  Only a CUDA(=HIP) implementation and a fake
(meta) implementation are registered -- like the reference there is no CPU
kernel, and there is deliberately no CPU fallback."""
import ctypes
import math
from typing import Callable, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import capi

try:
    _lib = torch.library.Library("quip_lib", "DEF")
except RuntimeError:  # namespace already defined in this process
    _lib = torch.library.Library("quip_lib", "FRAGMENT")

_SCHEMAS = {
    "hadamard": "(Tensor x, float scale) -> Tensor",
    "e8p_mm_origorder": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",
    "e8prvq3_mm_origorder": "(Tensor x, Tensor Qidxs, Tensor grid, Tensor grid2, float scale) -> Tensor",
    "e8prvq4_mm_origorder": "(Tensor x, Tensor Qidxs, Tensor grid, float scale) -> Tensor",
    "d4_mm_origorder": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",
    "hi_mm_origorder": "(Tensor x, Tensor Qidxs) -> Tensor",
    "decompress_e8p_origorder": "(Tensor Qidxs, Tensor grid) -> Tensor",
    "decompress_e8prvq3_origorder": "(Tensor Qidxs, Tensor grid, Tensor grid2, float scale) -> Tensor",
    "decompress_e8prvq4_origorder": "(Tensor Qidxs, Tensor grid, float scale) -> Tensor",
    "decompress_d4_origorder": "(Tensor Qidxs, Tensor grid) -> Tensor",
    "decompress_hi_origorder": "(Tensor Qidxs) -> Tensor",
    # fused Hadamard side of QuantLinear.forward (no reference counterpart: it
    # replaces the x*SU / pad / hadamard / hadK@ / *SV / +bias op sequence)
    "had_transform": "(Tensor x, int out_features, int n, int K, Tensor? had, bool transpose, "
                     "Tensor? pre, Tensor? pre2, Tensor? post, Tensor? bias, float scale) -> Tensor",
    # bs=1 decode path: input-side transform straight to int8 digit planes, and the GEMV on them
    "had_transform_planes": "(Tensor x, int n, int K, Tensor? had, bool transpose, Tensor? pre, float scale) -> Tensor",
    "e8p_gemv_planes": "(Tensor planes, Tensor Qidxs, Tensor grid) -> Tensor",
    # the same two transforms with decoder-block glue folded in (RMSNorm / SiLU*mul in, residual out)
    "had_transform_fused": "(Tensor x, int out_features, int n, int K, Tensor? had, bool transpose, Tensor? pre, "
                           "Tensor? pre2, Tensor? post, Tensor? bias, float scale, Tensor? residual, "
                           "Tensor? rms_weight, float rms_eps, Tensor? gate) -> Tensor",
    # grouped launches: the three stages of up to 3 QuantLinear modules reading the same activation
    "had_transform_planes_group": "(Tensor x, int n, int K, Tensor?[] had, bool transpose, Tensor?[] pre, "
                                  "float[] scale, Tensor? rms_weight, float rms_eps, Tensor? gate, "
                                  "float resid_scale=0.0) -> Tensor[]",
    "e8p_gemv_planes_group": "(Tensor[] planes, Tensor[] Qidxs, Tensor grid) -> Tensor[]",
    # rope + KV append + attention on the RAW GEMV outputs of q / k / v_proj (their K = 1 output transforms in the
    # launch's prologue): zs / posts = [q, k, v], scales = 1 / sqrt(n)
    "rope_attn_decode_z": "(Tensor[] zs, Tensor[] posts, float[] scales, Tensor cos, Tensor sin, Tensor pos, "
                          "Tensor(a!) kcache, Tensor(b!) vcache, Tensor? workspace=None, int window=0) -> Tensor",
    # M >= 32 (prefill): fused dequant + MFMA GEMM, x (M, k) fp16 -> (M, n) fp16; no dense W (csrc/e8p_prefill_gemm.hip)
    "e8p_mm_batched": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",
    # ... with the other codebooks' decode (argument meaning as the *_mm_skinny ops below)
    "e8prvq4_mm_batched": "(Tensor x, Tensor Qidxs, Tensor grid, float scale) -> Tensor",
    "e8prvq3_mm_batched": "(Tensor x, Tensor Qidxs, Tensor grid, Tensor grid2, float scale) -> Tensor",
    "d4_mm_batched": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",
    "hi_mm_batched": "(Tensor x, Tensor Qidxs) -> Tensor",
    # 2 <= M <= 32 rows in one pass over the codes, fp16 MFMA (csrc/e8p_skinny_gemm.hip)
    "e8p_mm_skinny": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",
    # the same for E8P12RVQ4B: int32 codes (main << 16 | residual), weights = fp16 fma(scale, residual, main)
    "e8prvq4_mm_skinny": "(Tensor x, Tensor Qidxs, Tensor grid, float scale) -> Tensor",
    "e8prvq3_mm_skinny": "(Tensor x, Tensor Qidxs, Tensor grid, Tensor grid2, float scale) -> Tensor",   # packed 3-byte codes
    "d4_mm_skinny": "(Tensor x, Tensor Qidxs, Tensor grid) -> Tensor",      # uint8 codes (n, k/4), the fp16 (256, 4) table
    "hi_mm_skinny": "(Tensor x, Tensor Qidxs) -> Tensor",                   # int32 codes (n, k/8), eight nibbles each
    # E8P12RVQ3B on the matrix-core GEMV: Qidxs = the checkpoint's 3-byte codes (int32 (n, 3k/32)), e81b_i8 = int8 (256, 8)
    "e8prvq3_gemv_planes_group": "(Tensor[] planes, Tensor[] Qidxs, Tensor grid, Tensor e81b_i8) -> Tensor[]",
    "d4_gemv_planes": "(Tensor planes, Tensor Qidxs, Tensor grid) -> Tensor",
    "d4_gemv_planes_group": "(Tensor[] planes, Tensor[] Qidxs, Tensor grid) -> Tensor[]",
    # 2..3 activation rows against ONE weight matrix: the grouped GEMV with the same codes for every row
    "e8p_mm_planes_rows": "(Tensor[] planes, Tensor Qidxs, Tensor grid) -> Tensor",
    # skinny GEMM on the matrix cores: M rows -> (M, planes_bytes) plane images -> (M, n); the GEMV op splits
    # the rows into passes of quip_e8p_gemv_max_rows(n, k) (5 for k <= 4096) rows each
    "had_transform_planes_rows": "(Tensor x, int n, int K, Tensor? had, bool transpose, Tensor? pre, float scale, "
                                 "Tensor? rms_weight, float rms_eps, Tensor? gate, float resid_scale=0.0) -> Tensor",
    "e8p_gemv_planes_rows": "(Tensor planes, Tensor Qidxs, Tensor grid) -> Tensor",
    # the same for the other table modes: 64 = D4 table (Qidxs uint8 (n, k/4)), 40 = E8P12RVQ3B (the 3-byte codes)
    "gemv_planes_rows_mode": "(Tensor planes, Tensor Qidxs, Tensor grid, Tensor? grid2, int mode) -> Tensor",
    # quantise-time nearest E8P12 codeword: X (N, 8) fp32 -> (vals (N, 8) fp32, idx (N) int64)
    "e8p_quantize": "(Tensor X, Tensor grid) -> (Tensor, Tensor)",
    # chain: output side of the producer module (z, its SV, residual) + input transforms of 1..3 consumers;
    # returns [h] + planes
    "had_chain_planes_group": "(Tensor z, Tensor z_post, Tensor? z_residual, float z_scale, int n, Tensor[] pre, "
                              "float[] scale, Tensor? rms_weight, float rms_eps, float resid_scale=0.0, int K=1, "
                              "Tensor? z_had=None, Tensor?[]? had=None) -> Tensor[]",
    "had_transform_group": "(Tensor[] x, int[] out_features, int n, int K, Tensor?[] had, bool transpose, "
                           "Tensor?[] pre2, Tensor?[] post, Tensor?[] bias, float[] scale, Tensor?[] residual, "
                           "Tensor?[] pre, Tensor? rms_weight, float rms_eps, int[]? ns=None) -> Tensor[]",
    # GEMV(s) with the input side computed in the prologue: [h_out]? + [y_i]; see quip_e8p_gemv_fused
    "e8p_gemv_fused": "(Tensor? x, Tensor? z, Tensor? post, Tensor? residual, Tensor? rms_weight, float rms_eps, "
                      "float z_scale, Tensor[] pre, float[] scale, Tensor[] Qidxs, Tensor grid) -> Tensor[]",
    # persistent decode engine, stage 1: GEMV[gate, up] -> output transforms -> SiLU product -> input transform of down
    # -> GEMV[down] in one launch (csrc/decode_engine.hip); returns down's raw product (1, hidden)
    "ffn_engine": "(Tensor planes_gate, Tensor planes_up, Tensor q_gate, Tensor q_up, Tensor q_down, Tensor had3, "
                  "Tensor sv_gate, Tensor sv_up, Tensor su_down, Tensor grid, Tensor(a!) workspace, float out_scale, "
                  "float in_scale, int K, Tensor? dbg=None) -> Tensor",
    # persistent decode engine, stage 2: n_layers decoder blocks of one token in one launch (csrc/decode_block.hip).
    # `layers` = the packed descriptors (decode.py builds them; they point at the KV caches, which the launch appends to)
    "block_engine": "(Tensor layers, Tensor h_in, Tensor pos, Tensor cos, Tensor sin, Tensor grid, Tensor(a!) workspace, "
                    "int n_layers, int max_len, float rms_eps, float attn_scale, Tensor? dbg=None, int dbg_layer=-1, "
                    "int codebook=0, float resid_scale=0.0, int shape=0, Tensor? grid2=None, "
                    # the KV caches the descriptors point into: row *pos of every block is written (declared here so that the
                    # mutation is visible to PyTorch; the kernel reaches them through the descriptors)
                    "Tensor(b!)? kcache=None, Tensor(c!)? vcache=None) -> Tensor",
    # decode-step glue between q/k/v_proj and o_proj: rope + KV-cache append + single-query attention
    "rope_attn_decode": "(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, Tensor(a!) kcache, "
                        "Tensor(b!) vcache, Tensor(c!)? workspace, int window=0) -> Tensor",   # window > 0: the last `window` positions only
    # greedy tail of the decode step: tok <- argmax(logits) (first maximum), pos += 1
    "argmax_step": "(Tensor logits, Tensor(a!) tok, Tensor(b!) pos) -> ()",
    "had_transform_planes_fused": "(Tensor x, int n, int K, Tensor? had, bool transpose, Tensor? pre, float scale, "
                                  "Tensor? rms_weight, float rms_eps, Tensor? gate, float resid_scale=0.0) -> Tensor",
}
for _name, _schema in _SCHEMAS.items():
    try:
        _lib.define(_name + _schema)
    except RuntimeError:
        pass  # already defined (e.g. the reference's register_lib was imported first)


# QUIP_POISON_OUTPUTS=1 (debug): every output tensor an op allocates is filled with a pattern (fp16 / fp32 NaN, 0xA5 bytes)
# before the launch instead of being left as _empty() memory, so a kernel that does not write all of its output,
# or that reads its output buffer, shows up as NaN / garbage instead of depending on what the allocator recycled.
import os as _os
_POISON = _os.environ.get("QUIP_POISON_OUTPUTS", "0") != "0"


def _empty(*shape, **kw):
    t = torch.empty(*shape, **kw)
    if _POISON and not torch.cuda.is_current_stream_capturing():
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        else:
            t.view(torch.uint8).fill_(0xA5)
    return t


def _stream(t: Tensor):
    return torch.cuda.current_stream(t.device).cuda_stream


def _ptr(t: Optional[Tensor]):
    return None if t is None else t.data_ptr()


def _need(cond, msg):
    if not cond:
        raise ValueError("quip_lib: " + msg)


# ---- the attention ops (here, batch_decode, chunk_attn, ragged_attn, paged_attn, qk_norm): one set of operand checks ----
_PAGE = 64              # positions per page of a paged cache (kPage, csrc/decode_glue.hip)
_MAX_SEGMENTS = 32      # QUIP_RAGGED_MAX_SEGMENTS


def _ptrs(*tensors):
    return [t.data_ptr() for t in tensors]


def _attn_call(entry, q, *args):
    """one attention entry point of the C ABI on q's device; the softmax scale is the caller's argument like every other"""
    with torch.cuda.device(q.device):
        capi.check(getattr(capi.lib(), entry)(*args), entry)


def _check_attn(what, layout, q, k, v, cos, sin, pos, kcache, vcache, table=None, pool_dtype=torch.float16):
    """The checks of the q / k / v / cos / sin / pos / cache family: dtype, contiguity, device and shape.  layout:
        "bs1"      q (heads, hd), k / v (kv_heads, hd), caches (kv_heads, max_len, hd), pos one element
        "chunk"    q (rows, heads, hd), k / v (rows, kv_heads, hd), caches and pos as bs1
        "batched"  q (B, heads, hd), k / v (B, kv_heads, hd), caches (B, kv_heads, max_len, hd), pos (B,)
        "ragged"   q (rows, heads, hd), k / v (rows, kv_heads, hd), caches and pos as batched
    With `table` (B, max_pages) int32 ("batched" / "ragged") the caches are pools (n_pages, kv_heads, 64, hd) of pool_dtype
    and max_len is the row count of cos.  -> (q.shape[0] or 1, heads, kv_heads, hd, max_len, B or 1)
    Two differences between the layouts are kept as they always were.  bs1 asks for CUDA tensors but does not compare
    their devices (and does not ask where cos / sin live): the bs = 1 decoder is the only caller and allocates all of
    them together.  Only chunk refuses zero rows itself; the other layouts leave an empty q to the entry point."""
    f16, bs1, slots, paged = torch.float16, layout == "bs1", layout in ("batched", "ragged"), table is not None
    if paged:     # (first: a pool of the other dtype is named as such whatever else is wrong)
        _need(kcache.dtype == pool_dtype and vcache.dtype == pool_dtype,
              f"{what}: the pools must be {'fp16' if pool_dtype == f16 else 'uint8 (e4m3fn bytes)'}")
    here = (lambda t: t.is_cuda) if bs1 else (lambda t: t.is_cuda and t.device == q.device)
    for t in (q, k, v, kcache, vcache):
        _need(t.dtype == (pool_dtype if t is kcache or t is vcache else f16) and t.is_contiguous() and here(t),
              f"{what}: fp16 contiguous tensors on one CUDA device")
    _need(all(t.dtype == torch.float32 and t.is_contiguous() and (bs1 or t.device == q.device) for t in (cos, sin)),
          "cos / sin must be contiguous float32" + ("" if bs1 else " on q's device"))
    _need(q.dim() == (2 if bs1 else 3) and kcache.dim() == (4 if slots else 3) and (not paged or table.dim() == 2),
          f"{what}: q ({'' if bs1 else 'B, ' if layout == 'batched' else 'rows, '}heads, hd), " +
          (f"pools (n_pages, kv_heads, {_PAGE}, hd), table (B, max_pages)" if paged else
           f"caches ({'B, ' if slots else ''}kv_heads, max_len, hd)"))
    lead, (heads, hd) = 1 if bs1 else q.shape[0], q.shape[-2:]
    if paged:
        kvh, (B, max_pages), max_len = kcache.shape[1], table.shape, cos.shape[0]
        cache_shape = (kcache.shape[0], kvh, _PAGE, hd)
        _need(table.dtype == torch.int32 and table.is_contiguous() and table.device == q.device,
              "table must be a contiguous int32 (B, max_pages) tensor on q's device")
    else:
        B, kvh, max_len = (1,) * (not slots) + tuple(kcache.shape[:-1])
        cache_shape = tuple(kcache.shape[:-1]) + (hd,)
    if slots:
        _need(pos.dtype == torch.int64 and tuple(pos.shape) == (B,) and pos.is_contiguous() and pos.device == q.device,
              "pos must be a contiguous int64 (B,) tensor on q's device")
        _need(layout != "batched" or lead == B, f"{what}: one q row per slot")
    else:
        _need(pos.dtype == torch.int64 and pos.numel() == 1 and (pos.is_cuda if bs1 else pos.device == q.device),
              "pos must be an int64 device scalar" + ("" if bs1 else " on q's device"))
        _need(lead >= 1, f"{what}: at least one row")
    kv_shape = (kvh, hd) if bs1 else (lead, kvh, hd)
    _need(tuple(k.shape) == kv_shape and tuple(v.shape) == kv_shape and tuple(kcache.shape) == cache_shape
          and tuple(vcache.shape) == cache_shape and tuple(cos.shape) == (max_len, hd) and tuple(sin.shape) == (max_len, hd)
          and (not paged or (cache_shape[0] >= 1 and max_pages >= 1 and 1 <= max_len <= max_pages * _PAGE)),
          f"{what}: shape mismatch")
    return lead, heads, kvh, hd, max_len, B


def _check_attn_workspace(workspace, q, batch, heads, hd):
    """the optional split-mode workspace of a decode-side launch: enough zeroed bytes on q's device; batch None: bs = 1"""
    if workspace is not None:
        _need(workspace.dtype == torch.uint8 and workspace.is_contiguous() and workspace.device == q.device
              and workspace.numel() >= capi.lib().quip_rope_attn_batched_workspace_bytes(batch or 1, heads, hd),
              "workspace: use rope_attn_workspace(heads, head_dim, device)" if batch is None else
              "workspace: use rope_attn_batched_workspace(batch, heads, head_dim, device)")


def _pack_segments(what, seg_slot, seg_rows, rows, B):
    """the segment lists of a ragged launch, checked -> (n, slots, counts), the two as ctypes int32 arrays"""
    seg_slot, seg_rows = [int(x) for x in seg_slot], [int(x) for x in seg_rows]
    n = len(seg_slot)
    _need(1 <= n <= _MAX_SEGMENTS and len(seg_rows) == n, f"{what}: 1 .. {_MAX_SEGMENTS} segments, one slot and one row count each")
    _need(all(r >= 1 for r in seg_rows) and sum(seg_rows) == rows, f"{what}: seg_rows >= 1 that sum to q's rows")
    _need(all(0 <= b < B for b in seg_slot) and len(set(seg_slot)) == n, f"{what}: distinct slots in [0, B)")
    return n, (ctypes.c_int32 * n)(*seg_slot), (ctypes.c_int32 * n)(*seg_rows)


def _chk_x(x: Tensor):
    _need(x.dim() == 2, "x must be 2-D (M, in)")
    _need(x.dtype == torch.float16, f"x must be float16, got {x.dtype}")
    return x.contiguous()


def _chk_lens(what, in_features, out_features, n, K, had=None, pre=None, pre2=None, post=None, bias=None,
              rms_weight=None):
    """element counts of the vectors a transform launch reads (a short vector would be read out of bounds):
    pre / rms_weight multiply the `in_features` inputs, pre2 the n transformed values, post / bias the
    `out_features` outputs, had is the (K, K) factor"""
    _need(0 < in_features <= n and 0 < out_features <= n and K >= 1 and n % K == 0,
          f"{what}: in_features {in_features} / out_features {out_features} must be in (0, n = {n}], K = {K} must divide n")
    for name, t, want in (("had", had, K * K), ("pre", pre, in_features), ("rms_weight", rms_weight, in_features),
                          ("pre2", pre2, n), ("post", post, out_features), ("bias", bias, out_features)):
        _need(t is None or t.numel() == want, f"{what}: {name} has {0 if t is None else t.numel()} elements, expected {want}")
    _need(K == 1 or had is not None, f"{what}: K = {K} needs the (K, K) factor")


def _chk_q(q: Tensor, dtype):
    _need(q.dim() == 2, "Qidxs must be 2-D")
    _need(q.dtype == dtype, f"Qidxs must be {dtype}, got {q.dtype}")
    return q.contiguous()


class _Entry:
    """a C entry point: resolved on the first call (the library loads on first use), then kept; a failure raises"""

    def __init__(self, name):
        self.name, self.fn = name, None

    def __call__(self, *args):
        if self.fn is None:
            self.fn = getattr(capi.lib(), self.name)
        capi.check(self.fn(*args), self.name)


def _args(tables):
    """the tables' ctypes arguments (the caller keeps `tables` alive over the call)"""
    return [t.data_ptr() if isinstance(t, Tensor) else t for t in tables]


# ---- hadamard ---------------------------------------------------------------------
_HAD_DTYPES = {torch.float16: 0, torch.bfloat16: 1, torch.float32: 2}     # QUIP_DTYPE_*


def _hadamard_cuda(x: Tensor, scale: float) -> Tensor:
    """fp16 / bf16 / fp32 like fast_hadamard_transform (register_lib.py:10-20); fp32 inside, output in x's dtype"""
    _need(x.dtype in _HAD_DTYPES, f"hadamard: float16 / bfloat16 / float32, got {x.dtype}")
    n = x.shape[-1]
    _need(n & (n - 1) == 0 and 0 < n <= 32768, f"hadamard length {n} must be a power of two <= 32768")
    xc = x.contiguous()
    y = torch.empty_like(xc)
    rows = xc.numel() // n
    if rows == 0:
        return y
    with torch.cuda.device(x.device):
        if x.dtype == torch.float16:
            capi.check(capi.lib().quip_hadamard_f16(xc.data_ptr(), y.data_ptr(), rows, n, float(scale),
                                                    _stream(x)), "quip_hadamard_f16")
        else:
            capi.check(capi.lib().quip_hadamard(xc.data_ptr(), y.data_ptr(), rows, n, float(scale),
                                                _HAD_DTYPES[x.dtype], _stream(x)), "quip_hadamard")
    return y


# ---- the transform ops: one problem builder, one operand check, one call --------------------------------------------------
HI_PLANES = float("inf")     # resid_scale value that selects the HI virtual-vector layout of the planes ops


def _layout(resid_scale):
    """the planes fields of a quip_had_problem from the ops' single float argument"""
    hi = resid_scale == HI_PLANES
    return {"resid_scale": 0.0 if hi else float(resid_scale), "planes_layout": 2 if hi else 0}


def _planes_numel(n, resid_scale=0.0):
    """quip_e8p_planes_bytes of the n digits, or of the 2n digits of a virtual-vector layout"""
    m = 2 * n if resid_scale != 0.0 else n
    return 3 * ((m + 511) // 512 * 512) + 16


_HAD_DEFAULTS = {"scale": 1.0, "rms_eps": 1e-5, "z_scale": 1.0}
_HAD_FIELDS = frozenset(f[0] for f in capi.HadProblem._fields_)


def _had_problem(**fields):
    """a capi.HadProblem by field name; a tensor stands for its address.  Unnamed fields take the defaults the header
    documents: scale = 1, rms_eps = 1e-5, z_scale = 1, the rest zero / NULL"""
    assert set(fields) <= _HAD_FIELDS, sorted(set(fields) - _HAD_FIELDS)
    return capi.HadProblem(**{**_HAD_DEFAULTS, **{k: _ptr(v) if v is None or isinstance(v, Tensor) else v for k, v in fields.items()}})


def _check_had(what, x, out_features, n, K, had=None, pre=None, pre2=None, post=None, bias=None, rms_weight=None,
               gate=None, residual=None):
    """The operand check of the family, for one problem on the rows x (from _chk_x): every optional tensor is fp16,
    contiguous and on x's device; the vectors have the lengths the launch reads (_chk_lens); gate has x's shape and
    residual the output's.  Before any library call."""
    for name, t in (("had", had), ("pre", pre), ("pre2", pre2), ("post", post), ("bias", bias), ("rms_weight", rms_weight),
                    ("gate", gate), ("residual", residual)):
        _need(t is None or (t.dtype == torch.float16 and t.is_contiguous() and t.device == x.device),
              f"{what}: {name} must be contiguous float16 on x's device")
    _need(gate is None or gate.shape == x.shape, f"{what}: gate must have x's shape")
    _need(residual is None or tuple(residual.shape) == (x.shape[0], out_features), f"{what}: residual must have the output's shape")
    _chk_lens(what, x.shape[1], out_features, n, K, had, pre, pre2, post, bias, rms_weight)


def _had_call(x, problems, planes, n, K, transpose, rows=None):
    """the problem-struct entry points: fp16 rows; planes of one row per problem (rows None); planes of the rows of one problem"""
    arr = (capi.HadProblem * len(problems))(*problems)
    L, tail = capi.lib(), (n, int(K), int(bool(transpose)), _stream(x))
    with torch.cuda.device(x.device):
        if not planes:
            capi.check(L.quip_had_transform_group_f16(arr, len(problems), rows, *tail), "quip_had_transform_group_f16")
        elif rows is None:
            capi.check(L.quip_had_transform_planes_group(arr, len(problems), *tail), "quip_had_transform_planes_group")
        else:
            capi.check(L.quip_had_transform_planes_rows(arr, rows, *tail), "quip_had_transform_planes_rows")


def _group_count(what, count, *lists):
    _need(1 <= count <= capi.MAX_GROUP and all(len(v) == count for v in lists),
          f"{what}: a group of 1..{capi.MAX_GROUP} problems, one entry per problem in every list")


def _had_transform_fused_cuda(x, out_features, n, K, had, transpose, pre, pre2, post, bias, scale, residual=None,
                              rms_weight=None, rms_eps=1e-5, gate=None, what="had_transform_fused"):
    xc = _chk_x(x)
    _check_had(what, xc, out_features, n, K, had, pre, pre2, post, bias, rms_weight, gate, residual)
    y = _empty((xc.shape[0], out_features), dtype=torch.float16, device=x.device)
    pr = _had_problem(x=xc, out=y, had=had, pre_scale=pre, pre_scale2=pre2, post_scale=post, bias=bias, residual=residual,
                      rms_weight=rms_weight, gate=gate, in_features=xc.shape[1], out_features=out_features,
                      scale=float(scale), rms_eps=float(rms_eps))
    _had_call(x, [pr], False, n, K, transpose, xc.shape[0])
    return y


def _had_transform_cuda(x, out_features, n, K, had, transpose, pre, pre2, post, bias, scale):
    return _had_transform_fused_cuda(x, out_features, n, K, had, transpose, pre, pre2, post, bias, scale, what="had_transform")


def _had_transform_planes_rows_cuda(x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate, resid_scale=0.0,
                                    what="had_transform_planes_rows", one_row=False):
    xc = _chk_x(x)
    _need(not one_row or xc.shape[0] == 1, f"{what} is the bs=1 path (one row)")
    _check_had(what, xc, n, n, K, had, pre, rms_weight=rms_weight, gate=gate)
    planes = _empty((_planes_numel(n, resid_scale),) if one_row else (xc.shape[0], _planes_numel(n, resid_scale)),
                    dtype=torch.uint8, device=x.device)
    pr = _had_problem(x=xc, out=planes, had=had, pre_scale=pre, rms_weight=rms_weight, gate=gate, in_features=xc.shape[1],
                      out_features=n, scale=float(scale), rms_eps=float(rms_eps), **_layout(resid_scale))
    _had_call(x, [pr], True, n, K, transpose, None if one_row else xc.shape[0])
    return planes


def _had_transform_planes_fused_cuda(x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate, resid_scale=0.0):
    return _had_transform_planes_rows_cuda(x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate, resid_scale,
                                           what="had_transform_planes_fused", one_row=True)


def _had_transform_planes_cuda(x, n, K, had, transpose, pre, scale):
    return _had_transform_planes_rows_cuda(x, n, K, had, transpose, pre, scale, None, 1e-5, None,
                                           what="had_transform_planes", one_row=True)


def _had_transform_planes_group_cuda(x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate, resid_scale=0.0):
    what = "had_transform_planes_group"
    xc = _chk_x(x)
    count = len(pre)
    _need(xc.shape[0] in (1, count), f"{what}: x has one row (shared) or one row per problem")
    _group_count(what, count, had, scale)
    for i in range(count):
        _check_had(what, xc, n, n, K, had[i], pre[i], rms_weight=rms_weight, gate=gate)
    outs = [_empty(_planes_numel(n, resid_scale), dtype=torch.uint8, device=x.device) for _ in range(count)]
    row = 2 * xc.shape[1] if xc.shape[0] == count and count > 1 else 0      # bytes from one problem's row to the next
    _had_call(x, [_had_problem(x=xc.data_ptr() + row * i, out=outs[i], had=had[i], pre_scale=pre[i], rms_weight=rms_weight,
                               gate=None if gate is None else gate.data_ptr() + row * i, in_features=xc.shape[1],
                               out_features=n, scale=float(scale[i]), rms_eps=float(rms_eps), **_layout(resid_scale))
                  for i in range(count)], True, n, K, transpose)
    return outs


def _had_chain_planes_group_cuda(z, z_post, z_residual, z_scale, n, pre, scale, rms_weight, rms_eps, resid_scale=0.0,
                                 K=1, z_had=None, had=None):
    """K > 1 (n = K * L): z_had is the producer's (K, K) had_right, had[i] consumer i's had_left (applied transposed);
    z_scale and scale then carry 1 / sqrt(L)"""
    what = "had_chain_planes_group"
    zc = _chk_x(z)
    count = len(pre)
    _need(zc.shape == (1, n), f"{what} is the bs=1 path: z must be (1, n)")
    had = list(had) if had is not None else [None] * count
    _group_count(what, count, scale, had)
    _need(K == 1 or z_had is not None, f"{what}: K = {K} needs the producer's (K, K) factor")
    for i in range(count):
        _check_had(what, zc, n, n, K, had[i], pre[i], post=z_post, rms_weight=rms_weight, residual=z_residual)
    _check_had(what + " (producer)", zc, n, n, K, z_had if K > 1 else None)
    outs = [_empty(_planes_numel(n, resid_scale), dtype=torch.uint8, device=z.device) for _ in range(count)]
    h = _empty((1, n), dtype=torch.float16, device=z.device)
    factors = {} if K == 1 else {"z_had": z_had}
    _had_call(z, [_had_problem(out=outs[i], had=had[i] if K > 1 else None, pre_scale=pre[i], rms_weight=rms_weight,
                               in_features=n, out_features=n, scale=float(scale[i]), rms_eps=float(rms_eps), z=zc,
                               z_post_scale=z_post, z_residual=z_residual, h_out=h, z_scale=float(z_scale), **factors,
                               **_layout(resid_scale)) for i in range(count)], True, n, K, True)
    return [h] + outs


def _had_transform_group_cuda(x, out_features, n, K, had, transpose, pre2, post, bias, scale, residual, pre,
                              rms_weight, rms_eps, ns=None):
    what = "had_transform_group"
    count = len(x)
    _group_count(what, count, out_features, had, pre2, post, bias, scale, residual, pre)
    xs = [_chk_x(t) for t in x]
    rows = xs[0].shape[0]
    _need(all(t.shape[0] == rows and t.device == xs[0].device for t in xs), f"{what}: group inputs must share rows / device")
    _need(ns is not None or all(t.shape == xs[0].shape for t in xs), f"{what}: group inputs must share a shape (or pass ns)")
    _need(ns is None or (len(ns) == count and K == 1 and rms_weight is None),
          f"{what}: ns: one width per problem, K == 1, no rms_weight")
    for i in range(count):
        _check_had(what, xs[i], int(out_features[i]), int(ns[i]) if ns is not None else n, K, had[i], pre[i], pre2[i], post[i],
                   bias[i], rms_weight, residual=residual[i])
    outs = [_empty((rows, int(o)), dtype=torch.float16, device=xs[0].device) for o in out_features]
    _had_call(xs[0], [_had_problem(x=xs[i], out=outs[i], had=had[i], pre_scale=pre[i], pre_scale2=pre2[i], post_scale=post[i],
                                   bias=bias[i], residual=residual[i], rms_weight=rms_weight, in_features=xs[i].shape[1],
                                   out_features=int(out_features[i]), scale=float(scale[i]), rms_eps=float(rms_eps),
                                   n=int(ns[i]) if ns is not None else 0) for i in range(count)], False, n, K, transpose, rows)
    return outs


def _argmax_step_cuda(logits, tok, pos):
    _need(logits.dtype == torch.float16 and logits.is_contiguous() and logits.dim() <= 2
          and (logits.dim() == 1 or logits.shape[0] == 1), "argmax_step: logits must be contiguous float16 (1, n)")
    _need(tok.dtype == torch.int64 and pos.dtype == torch.int64 and tok.numel() >= 1 and pos.numel() >= 1
          and tok.device == logits.device and pos.device == logits.device, "tok / pos: int64 on the logits' device")
    with torch.cuda.device(logits.device):
        capi.check(capi.lib().quip_argmax_step_f16(logits.data_ptr(), logits.numel(), tok.data_ptr(), pos.data_ptr(),
                                                   _stream(logits)), "quip_argmax_step_f16")


def _e8p_quantize_cuda(X, grid):
    _need(X.dim() == 2 and X.shape[1] == 8 and X.dtype == torch.float32 and X.is_contiguous(),
          "e8p_quantize: X must be contiguous float32 (N, 8)")
    g = _grid_i64(grid, X)
    vals = torch.empty_like(X)
    idx = _empty(X.shape[0], dtype=torch.int64, device=X.device)
    with torch.cuda.device(X.device):
        capi.check(capi.lib().quip_e8p_quantize_f32(X.data_ptr(), X.shape[0], g.data_ptr(), vals.data_ptr(),
                                                    idx.data_ptr(), _stream(X)), "quip_e8p_quantize_f32")
    return vals, idx


def _e8p_mm_planes_rows_cuda(planes, Qidxs, grid):
    count = len(planes)
    _need(1 <= count <= capi.MAX_GROUP, "1..3 rows")
    _need(Qidxs.dtype == torch.int16 and Qidxs.is_contiguous(), "Qidxs must be contiguous int16 (n, k/8)")
    n, k = Qidxs.shape[0], Qidxs.shape[1] * 8
    dev = Qidxs.device
    out = _empty((count, n), dtype=torch.float16, device=dev)
    vp = ctypes.c_void_p * count
    ns = (ctypes.c_int32 * count)(*([n] * count))
    g = _grid_i64(grid, Qidxs)
    with torch.cuda.device(dev):
        capi.check(capi.lib().quip_e8p_gemv_planes_group(
            vp(*[p.data_ptr() for p in planes]), vp(*([Qidxs.data_ptr()] * count)), g.data_ptr(),
            vp(*[out.data_ptr() + 2 * n * i for i in range(count)]), ns, count, k, _stream(out)),
            "quip_e8p_gemv_planes_group (rows)")
    return out


_GEMV_WS = {}        # (device type, index, stream handle) -> zeroed int32 workspace
_GEMV_WS_RETIRED = []   # superseded workspaces: captured hipGraphs may still hold their pointers, so they are never freed


class _RawWorkspace:
    """device memory from hipMalloc itself, not from torch's caching allocator: a buffer that is created on first use and lives
    for the whole process must not come out of whatever memory pool is current at that moment -- inside
    torch.compile(mode="reduce-overhead") (HF's generate with a static cache compiles the forward that way) that is the
    cudagraph trees' private pool, which refuses live allocations it did not hand out as outputs"""
    _hip = None

    def __init__(self, nbytes, dev):
        if _RawWorkspace._hip is None:
            _RawWorkspace._hip = ctypes.CDLL("libamdhip64.so")
        hip = _RawWorkspace._hip
        p = ctypes.c_void_p()
        with torch.cuda.device(dev):
            rc = hip.hipMalloc(ctypes.byref(p), ctypes.c_size_t(nbytes))
            if rc != 0 or not p.value:
                raise RuntimeError(f"hipMalloc({nbytes}) failed: {rc}")
            rc = hip.hipMemset(p, 0, ctypes.c_size_t(nbytes))
            if rc != 0:
                raise RuntimeError(f"hipMemset failed: {rc}")
        self.ptr, self.nbytes = int(p.value), int(nbytes)

    def data_ptr(self):
        return self.ptr

    def numel(self):                 # int32 words, like the tensor this replaces
        return self.nbytes // 4

    def read(self):
        """the contents as an int32 CPU tensor (tests: a launch leaves its workspace zeroed); synchronises the device"""
        out = torch.empty(self.nbytes // 4, dtype=torch.int32)
        torch.cuda.synchronize()
        rc = _RawWorkspace._hip.hipMemcpy(ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(self.ptr), ctypes.c_size_t(self.nbytes), 2)
        if rc != 0:
            raise RuntimeError(f"hipMemcpy failed: {rc}")
        return out

    def abs(self):                   # (the tensor methods the tests use on a workspace)
        return self.read().abs()


def _gemv_workspace(dev, n_total):
    """zeroed int32 scratch for K-split GEMV launches: ONE PER (device, stream) -- two streams running such launches at
    the same time must not add into the same accumulators and arrival counters -- kept for the life of the process
    (captured hipGraphs hold its pointer); every launch leaves it zeroed.  A workspace that has to grow is replaced,
    never freed: the old one stays alive for the graphs that captured it.  Raw device memory (_RawWorkspace) unless a stream
    capture is under way (hipMalloc is not allowed there: torch's allocator, which knows the capture's pool, serves it)."""
    need = capi.lib().quip_e8p_gemv_workspace_bytes(int(n_total))
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _GEMV_WS.get(key)
    if ws is None or ws.numel() * 4 < need:
        if ws is not None:
            _GEMV_WS_RETIRED.append(ws)
        nbytes = max(need, 4 << 20)
        if torch.cuda.is_current_stream_capturing():
            with torch.cuda.stream(torch.cuda.current_stream(dev)):
                ws = torch.zeros(nbytes // 4, dtype=torch.int32, device=dev)
        else:
            ws = _RawWorkspace(nbytes, dev)
        _GEMV_WS[key] = ws
    return ws


# ---- the stand-alone bs=1 GEMV on digit planes, one spec per table mode: (planes, Qidxs, tables) -> outs ------------------
class _GemvMode(NamedTuple):
    entry: _Entry             # the group entry point with a workspace
    qdtype: torch.dtype
    cols: Tuple[int, int]     # in features per code column, as (numerator, denominator)
    virtual: int              # the planes hold quip_e8p_planes_bytes(virtual * in features)
    qmsg: str
    tables: Callable          # (planes[0], *the op's table arguments) -> the entry point's table arguments
    rows_mode: int            # the table-mode number of rows mode (quip_gemv_max_rows_mode, quip_gemv_planes_rows_mode)


def _e81b_i8(e81b_i8, ref):
    _need(e81b_i8.dtype == torch.int8 and tuple(e81b_i8.shape) == (256, 8) and e81b_i8.is_contiguous()
          and e81b_i8.device == ref.device, "e81b_i8 must be the contiguous int8 (256, 8) table")
    return e81b_i8


def _d4_grid(grid):
    _need(grid.dtype == torch.float16 and grid.is_contiguous() and tuple(grid.shape) == (256, 4),
          "D4 grid must be the contiguous fp16 (256, 4) table")
    return grid


_GEMV_E8P = _GemvMode(_Entry("quip_e8p_gemv_planes_group_ws"), torch.int16, (8, 1), 1,
                      "Qidxs must be contiguous int16 (n, k/8) with a common k", lambda ref, grid: (_grid_i64(grid, ref),),
                      0)
# (HI runs in the D4 table mode through its virtual layout: its uint8 view already counts 2 k weights per row)
_GEMV_D4 = _GemvMode(_Entry("quip_d4_gemv_planes_group_ws"), torch.uint8, (4, 1), 1,
                     "Qidxs must be contiguous uint8 (n, k/4) with a common k", lambda ref, grid: (_d4_grid(grid),),
                     64)
_GEMV_RVQ3 = _GemvMode(_Entry("quip_e8prvq3_gemv_planes_group_ws"), torch.int32, (32, 3), 2,
                       "Qidxs must be the checkpoint's contiguous int32 (n, 3 k / 32) tensors (3-byte codes) with a common k",
                       lambda ref, grid, e81b_i8: (_grid_i64(grid, ref), _e81b_i8(e81b_i8, ref)),
                       40)


def _gemv(mode, planes, Qidxs, *tables):
    count = len(planes)
    _need(1 <= count <= capi.MAX_GROUP and len(Qidxs) == count, "group of 1..3 problems")
    num, den = mode.cols
    _need(Qidxs[0].shape[1] * num % den == 0, mode.qmsg)
    k = Qidxs[0].shape[1] * num // den
    dev = planes[0].device
    nbytes = capi.lib().quip_e8p_planes_bytes(mode.virtual * k)
    for pl, q in zip(planes, Qidxs):
        _need(q.dtype == mode.qdtype and q.is_contiguous() and q.shape[1] * num == k * den and q.device == dev, mode.qmsg)
        _need(pl.dtype == torch.uint8 and pl.is_contiguous() and pl.device == dev and pl.numel() >= nbytes,
              f"planes must be contiguous uint8 images of at least quip_e8p_planes_bytes({mode.virtual * k}) = {nbytes} bytes")
    tabs = mode.tables(planes[0], *tables)
    outs = [_empty((1, q.shape[0]), dtype=torch.float16, device=dev) for q in Qidxs]
    vp = ctypes.c_void_p * count
    ns = (ctypes.c_int32 * count)(*[q.shape[0] for q in Qidxs])
    ws = _gemv_workspace(dev, sum(q.shape[0] for q in Qidxs))
    with torch.cuda.device(dev):
        mode.entry(vp(*[p.data_ptr() for p in planes]), vp(*[q.data_ptr() for q in Qidxs]), *_args(tabs),
                   vp(*[o.data_ptr() for o in outs]), ns, count, k, ws.data_ptr(), ws.numel() * 4, _stream(planes[0]))
    return outs


_GEMV_ROWS = _Entry("quip_gemv_planes_rows_mode")      # (mode 0 is what quip_e8p_gemv_planes_rows forwards to)


def _gemv_rows(mode, planes, Qidxs, *tables):
    """rows mode: the (rows, planes bytes) images of had_transform_planes_rows against one matrix -> (rows, n), in passes of
    quip_gemv_max_rows_mode(n, k, mode) rows over the codes (k: the weights of a row as the kernel sees them)"""
    L = capi.lib()
    num, den = mode.cols
    _need(Qidxs.dim() == 2 and Qidxs.dtype == mode.qdtype and Qidxs.is_contiguous() and Qidxs.shape[1] * num % den == 0,
          mode.qmsg)
    n, k = Qidxs.shape[0], mode.virtual * (Qidxs.shape[1] * num // den)
    _need(planes.dim() == 2 and planes.dtype == torch.uint8 and planes.is_contiguous()
          and planes.shape[1] == L.quip_e8p_planes_bytes(k) and planes.device == Qidxs.device,
          "planes must be the (rows, quip_e8p_planes_bytes(k)) uint8 images of had_transform_planes_rows")
    tabs = _args(mode.tables(planes, *tables))
    rows = planes.shape[0]
    per = L.quip_gemv_max_rows_mode(n, k, mode.rows_mode)
    out = _empty((rows, n), dtype=torch.float16, device=Qidxs.device)
    if per < 1:
        # rows longer than rows mode holds in LDS (k > 28672: the 2k-wide virtual rows at the 70B down_proj width): one
        # bs=1 launch per row through the stand-alone GEMV (the K-splitting kernel) -- the same exact integer sums
        if mode is _GEMV_E8P and (rows == 0 or n == 0):     # (E8P12's op takes an empty problem; the other two refuse it)
            return out
        return torch.cat([_gemv(mode, [planes[r]], [Qidxs], *tables)[0] for r in range(rows)])
    grid, grid2 = (tabs + [None])[:2]                       # (grid2: the E81B table of mode 40, else NULL)
    with torch.cuda.device(Qidxs.device):
        for r0 in range(0, rows, per):
            _GEMV_ROWS(planes[r0].data_ptr(), Qidxs.data_ptr(), grid, grid2, out[r0].data_ptr(), min(per, rows - r0), n, k,
                       mode.rows_mode, _stream(out))
    return out


def _gemv_planes_rows_mode_cuda(planes, Qidxs, grid, grid2, mode):
    _need(mode in (64, 40), "mode: 64 (D4 table) or 40 (E8P12RVQ3B tables)")
    _need(mode == 64 or grid2 is not None, "grid2 must be the contiguous int8 (256, 8) E81B table")
    return _gemv_rows(_GEMV_D4, planes, Qidxs, grid) if mode == 64 else _gemv_rows(_GEMV_RVQ3, planes, Qidxs, grid, grid2)


def _e8p_gemv_planes_cuda(planes, Qidxs, grid):
    Qc = _chk_q(Qidxs, torch.int16)
    if Qc.shape[0] == 0:         # (the single-matrix entry point takes an empty matrix)
        return _empty((1, 0), dtype=torch.float16, device=Qidxs.device)
    return _gemv(_GEMV_E8P, [planes], [Qc], grid)[0]


def _e8p_gemv_fused_cuda(x, z, post, residual, rms_weight, rms_eps, z_scale, pre, scale, Qidxs, grid):
    count = len(Qidxs)
    _need(1 <= count <= capi.MAX_GROUP and len(pre) == count and len(scale) == count, "group of 1..3 problems")
    k = Qidxs[0].shape[1] * 8
    src = z if z is not None else x
    _need(src is not None and src.numel() == k and src.dtype == torch.float16 and src.is_contiguous(),
          "x / z must be a contiguous fp16 vector of k elements")
    dev = src.device
    for q in Qidxs:
        _need(q.dtype == torch.int16 and q.is_contiguous() and q.shape[1] * 8 == k and q.device == dev,
              "Qidxs must be contiguous int16 (n, k/8) with a common k")
    for t in [post, residual, rms_weight] + list(pre):
        _need(t is None or (t.numel() == k and t.dtype == torch.float16 and t.is_contiguous() and t.device == dev),
              "vectors must be contiguous fp16 of k elements")
    _need(z is None or post is not None, "post (the producer's SV) is required with z")
    outs = [_empty((1, q.shape[0]), dtype=torch.float16, device=dev) for q in Qidxs]
    h_out = _empty((1, k), dtype=torch.float16, device=dev) if z is not None else None
    fin = capi.GemvFusedIn()
    fin.x, fin.z, fin.post_scale, fin.residual = _ptr(x), _ptr(z), _ptr(post), _ptr(residual)
    fin.h_out, fin.rms_weight = _ptr(h_out), _ptr(rms_weight)
    for i in range(count):
        fin.pre_scale[i] = pre[i].data_ptr()
        fin.scale[i] = float(scale[i])
    fin.z_scale, fin.rms_eps = float(z_scale), float(rms_eps)
    vp = ctypes.c_void_p * count
    ns = (ctypes.c_int32 * count)(*[q.shape[0] for q in Qidxs])
    g = _grid_i64(grid, src)
    with torch.cuda.device(dev):
        capi.check(capi.lib().quip_e8p_gemv_fused(
            ctypes.byref(fin), vp(*[q.data_ptr() for q in Qidxs]), g.data_ptr(),
            vp(*[o.data_ptr() for o in outs]), ns, count, k, _stream(src)), "quip_e8p_gemv_fused")
    return ([h_out] if h_out is not None else []) + outs


def ffn_engine_supported(hidden, n_ffn, K):
    return bool(capi.lib().quip_ffn_engine_supported(int(hidden), int(n_ffn), int(K)))


def ffn_engine_workspace(n_ffn, K, device):
    """hand-off area of the engine launches of one decoder (zeroed once; launches sharing it must be stream ordered)"""
    return torch.zeros(capi.lib().quip_ffn_engine_workspace_bytes(int(n_ffn), int(K)), dtype=torch.uint8, device=device)


def ffn_engine_status(workspace):
    """0, or the code of the wait that gave up in an engine launch on this workspace (synchronises)"""
    return int(workspace[:8].view(torch.int32)[1].item())


def _ffn_engine_cuda(planes_gate, planes_up, q_gate, q_up, q_down, had3, sv_gate, sv_up, su_down, grid, workspace,
                     out_scale, in_scale, K, dbg=None):
    dev = planes_gate.device
    n_ffn, hidden = q_gate.shape[0], q_gate.shape[1] * 8
    for q in (q_gate, q_up, q_down):
        _need(q.dtype == torch.int16 and q.is_contiguous() and q.device == dev, "Qidxs must be contiguous int16")
    _need(q_up.shape == q_gate.shape and q_down.shape == (hidden, n_ffn // 8), "gate / up (n_ffn, hidden / 8), down (hidden, n_ffn / 8)")
    _need(ffn_engine_supported(hidden, n_ffn, K), f"ffn_engine: shape (hidden {hidden}, n_ffn {n_ffn}, K {K}) not supported")
    kp = (hidden + 511) // 512 * 512
    for pl in (planes_gate, planes_up):
        _need(pl.dtype == torch.uint8 and pl.is_contiguous() and pl.numel() == 3 * kp + 16 and pl.device == dev,
              "planes must be uint8 images of 3 Kp + 16 bytes")
    kkp, kp16 = (K * K + 7) // 8 * 8, (K + 15) // 16 * 16
    _need(had3.dtype == torch.float16 and had3.is_contiguous() and had3.numel() == 2 * kkp + kp16 * kp16
          and had3.device == dev, "had3 must be the fp16 pack of qlinear._engine_had3")
    for v in (sv_gate, sv_up, su_down):
        _need(v.dtype == torch.float16 and v.is_contiguous() and v.numel() == n_ffn and v.device == dev,
              "sv_gate / sv_up / su_down must be fp16 vectors of n_ffn elements")
    _need(workspace.dtype == torch.uint8 and workspace.device == dev
          and workspace.numel() >= capi.lib().quip_ffn_engine_workspace_bytes(n_ffn, K), "workspace too small")
    g = _grid_i64(grid, planes_gate)
    out = _empty((1, hidden), dtype=torch.float16, device=dev)
    a = capi.FfnEngineArgs(q_gate.data_ptr(), q_up.data_ptr(), q_down.data_ptr(), planes_gate.data_ptr(),
                           planes_up.data_ptr(), had3.data_ptr(), sv_gate.data_ptr(), sv_up.data_ptr(),
                           su_down.data_ptr(), out.data_ptr(), g.data_ptr(), workspace.data_ptr(), _ptr(dbg),
                           float(out_scale), float(in_scale), hidden, n_ffn, int(K))
    with torch.cuda.device(dev):
        capi.check(capi.lib().quip_ffn_engine(ctypes.byref(a), _stream(planes_gate)), "quip_ffn_engine")
    return out


def block_engine_supported(hidden, heads, kv_heads, head_dim, n_ffn, K):
    return bool(capi.lib().quip_block_engine_supported(int(hidden), int(heads), int(kv_heads), int(head_dim), int(n_ffn), int(K)))


def _block_engine_ws_bytes(shape):
    L = capi.lib()
    return (L.quip_block_engine_gqa_workspace_bytes() if shape == 1 else
            L.quip_block_engine_g8_workspace_bytes() if shape == 2 else L.quip_block_engine_workspace_bytes())


def block_engine_workspace(device, shape=0):
    return torch.zeros(_block_engine_ws_bytes(shape), dtype=torch.uint8, device=device)


def block_engine_g8_supported(hidden, heads, kv_heads, head_dim, n_ffn, K):
    """the 4096-wide grouped-query shape of Llama-3-8B / Mistral-7B (32 / 8 heads of 128, n_ffn 14336, K = 7) on the persistent launch"""
    return bool(capi.lib().quip_block_engine_g8_supported(int(hidden), int(heads), int(kv_heads), int(head_dim), int(n_ffn), int(K)))


def block_engine_gqa_supported(hidden, heads, kv_heads, head_dim, n_ffn, K):
    return bool(capi.lib().quip_block_engine_gqa_supported(int(hidden), int(heads), int(kv_heads), int(head_dim), int(n_ffn), int(K)))


def _block_engine_cuda(layers, h_in, pos, cos, sin, grid, workspace, n_layers, max_len, rms_eps, attn_scale, dbg=None,
                       dbg_layer=-1, codebook=0, resid_scale=0.0, shape=0, grid2=None, kcache=None, vcache=None):
    dev = h_in.device
    lb = capi.lib().quip_block_engine_layer_bytes()
    _need(layers.dtype == torch.uint8 and layers.is_contiguous() and layers.numel() >= n_layers * lb and layers.device == dev,
          "layers must be the packed descriptors (uint8, n_layers x 256 bytes) on the device")
    _need(shape in (0, 1, 2), "shape: 0 (hidden 4096, multi-head), 1 (hidden 8192, grouped-query) or 2 (hidden 4096, grouped-query)")
    hid = 8192 if shape == 1 else 4096
    _need(h_in.dtype == torch.float16 and h_in.is_contiguous() and h_in.numel() == hid, f"h_in: fp16 [{hid}]")
    _need(pos.dtype == torch.int64 and pos.numel() == 1 and pos.device == dev, "pos: int64 device scalar")
    for t in (cos, sin):
        _need(t.dtype == torch.float32 and t.is_contiguous() and t.shape == (max_len, 128) and t.device == dev,
              "cos / sin: fp32 [max_len, 128]")
    need_ws = _block_engine_ws_bytes(shape)
    _need(workspace.dtype == torch.uint8 and workspace.device == dev and workspace.numel() >= need_ws, "workspace too small")
    if codebook in (1, 3):      # D4 / HI: the fp16 (256, 4) table (HI: of a code byte) -- 2 KB like grid_packed_abs
        g = _d4_grid_f16(grid)
        _need(g.device == dev and g.numel() == 1024, "D4 / HI grid: fp16 (256, 4) on the device")
    else:
        g = _grid_i64(grid, h_in)
    if codebook == 4:           # E8P12RVQ3B: the E81B table as int8 (256, 8) = 4 r
        _need(grid2 is not None and grid2.dtype == torch.int8 and grid2.is_contiguous() and grid2.numel() == 2048 and grid2.device == dev,
              "grid2: the E81B table as int8 (256, 8) on the device")
    out = torch.empty_like(h_in)
    a = capi.BlockEngineArgs(layers.data_ptr(), h_in.data_ptr(), out.data_ptr(), pos.data_ptr(), cos.data_ptr(),
                             sin.data_ptr(), g.data_ptr(), workspace.data_ptr(), _ptr(dbg), int(n_layers), int(max_len),
                             int(dbg_layer), float(rms_eps), float(attn_scale), int(codebook), float(resid_scale), int(shape),
                             _ptr(grid2) if codebook == 4 else None)
    with torch.cuda.device(dev):
        rc = capi.lib().quip_block_engine(ctypes.byref(a), _stream(h_in))
        # (shape 1, dbg_layer == -2: the measurement mode answers QUIP_NO_RESULT = 1 -- the caller asked for exactly that)
        if not (rc == 1 and shape == 1 and int(dbg_layer) == -2):
            capi.check(rc, "quip_block_engine")
    return out


def rope_attn_workspace(heads, head_dim, device):
    """zeroed scratch for the split (long context) mode of rope_attn_decode; allocate once, reuse"""
    return torch.zeros(capi.lib().quip_rope_attn_workspace_bytes(heads, head_dim), dtype=torch.uint8, device=device)


def _rope_attn_decode_cuda(q, k, v, cos, sin, pos, kcache, vcache, workspace=None, window=0):
    """q (heads, hd), k / v (kv_heads, hd) fp16; cos / sin (max_len, hd) fp32; pos int64 device scalar;
    kcache / vcache (kv_heads, max_len, hd) fp16 (row pos is written) -> (heads, hd) fp16"""
    _, heads, kvh, hd, max_len, _ = _check_attn("rope_attn_decode", "bs1", q, k, v, cos, sin, pos, kcache, vcache)
    _check_attn_workspace(workspace, q, None, heads, hd)
    out = torch.empty_like(q)
    _attn_call("quip_rope_attn_decode_window_f16", q, *_ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), heads, kvh, hd,
               max_len, 1.0 / math.sqrt(hd), int(window), _ptr(workspace), _stream(q))
    return out


def rope_attn_decode_z_supported(heads, kv_heads, head_dim):
    return bool(capi.lib().quip_rope_attn_decode_z_supported(heads, kv_heads, head_dim))


def _rope_attn_decode_z_cuda(zs, posts, scales, cos, sin, pos, kcache, vcache, workspace=None, window=0):
    """zs / posts: the raw GEMV outputs (1, n) or (n,) and SV vectors (n,) of q / k / v_proj, fp16; the rest as
    rope_attn_decode -> (heads, hd) fp16"""
    _need(len(zs) == 3 and len(posts) == 3 and len(scales) == 3, "rope_attn_decode_z: q, k, v")
    kvh, max_len, hd = kcache.shape
    n = zs[0].numel()
    heads = n // hd
    for i, t in enumerate(list(zs) + list(posts)):
        _need(t.dtype == torch.float16 and t.is_contiguous() and t.is_cuda and t.numel() == (n if i % 3 == 0 else kvh * hd),
              "rope_attn_decode_z: fp16 contiguous CUDA vectors, heads * head_dim (q) / kv_heads * head_dim (k, v) long")
    for t in (kcache, vcache):
        _need(t.dtype == torch.float16 and t.is_contiguous() and t.is_cuda, "rope_attn_decode_z: fp16 caches")
    _need(heads * hd == n and rope_attn_decode_z_supported(heads, kvh, hd),
          "rope_attn_decode_z: needs heads == kv_heads and heads * head_dim a power of two in 256..4096, or 64 / 32 heads "
          "of 128 on 8 KV heads")
    _need(cos.dtype == torch.float32 and sin.dtype == torch.float32 and cos.is_contiguous() and sin.is_contiguous()
          and tuple(cos.shape) == (max_len, hd) and tuple(sin.shape) == (max_len, hd), "cos / sin: float32 (max_len, hd)")
    _need(pos.dtype == torch.int64 and pos.numel() == 1 and pos.is_cuda, "pos must be an int64 device scalar")
    _need(tuple(vcache.shape) == tuple(kcache.shape), "cache shapes differ")
    out = _empty((heads, hd), dtype=torch.float16, device=kcache.device)
    _check_attn_workspace(workspace, kcache, None, heads, hd)
    zp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in zs])
    pp = (ctypes.c_void_p * 3)(*[t.data_ptr() for t in posts])
    sc = (ctypes.c_float * 3)(*[float(x) for x in scales])
    _attn_call("quip_rope_attn_decode_z_window_f16", kcache, zp, pp, sc, *_ptrs(cos, sin, pos, kcache, vcache, out), heads, kvh,
               hd, max_len, 1.0 / math.sqrt(hd), int(window), _ptr(workspace), _stream(kcache))
    return out


def e8p_mm_batched_supported(m, n, k):
    """shapes the fused batched product takes (quip_e8p_mm_batched)"""
    return m >= 1 and n >= 2 and n % 2 == 0 and k >= 64 and k % 64 == 0


def e8p_mm_skinny_supported(m, n, k):
    """(rows beyond 32 run as chunks of 32 in the same launch)"""
    return 1 <= m <= 32 * 65535 and n >= 2 and n % 2 == 0 and k >= 128 and k % 128 == 0


def _grid_i64(grid: Tensor, x: Tensor):
    _need(grid.dtype == torch.int64 and grid.numel() == 256, "grid_packed_abs must be int64[256]")
    _need(grid.device == x.device, "grid and x must be on the same device")
    return grid.contiguous()


def _e81b_packed(grid2: Tensor, x: Tensor):
    _need(grid2.dtype == torch.int32 and grid2.numel() == 256, "e81b_grid_packed must be int32[256]")
    _need(grid2.device == x.device, "grid2 and x must be on the same device")
    return grid2.contiguous()


def _d4_grid_f16(grid: Tensor):
    # the reference kernel reinterprets `grid` as uint64[256], i.e. it silently
    # requires fp16 (origin_order.cu:794-805); cast explicitly here.
    _need(grid.numel() == 1024, "D4 grid must be (256, 4)")
    return grid.to(torch.float16).contiguous()


# ---- the five codebooks: one description each, one implementation per op family ------------------------------------
class _Codebook(NamedTuple):
    qdtype: torch.dtype
    cols: Tuple[int, int]     # in features per code column, as (numerator, denominator)
    tables: Callable          # (x, *the op's table arguments) -> the entry point's table arguments (tensors / floats)


_CODEBOOKS = {
    "e8p": _Codebook(torch.int16, (8, 1), lambda x, grid: (_grid_i64(grid, x),)),
    "e8prvq4": _Codebook(torch.int32, (8, 1), lambda x, grid, scale: (_grid_i64(grid, x), float(scale))),
    "e8prvq3": _Codebook(torch.int32, (32, 3), lambda x, grid, grid2, scale: (_grid_i64(grid, x), _e81b_packed(grid2, x),
                                                                              float(scale))),
    "d4": _Codebook(torch.uint8, (4, 1), lambda x, grid: (_d4_grid_f16(grid),)),
    "hi": _Codebook(torch.int32, (8, 1), lambda x: ()),
}


def _operands(what, cb, x, Qidxs):
    """x (M, k) fp16 and the codes of an (n, k) matrix -> (x, Qidxs) contiguous, m, n, k"""
    xc = _chk_x(x)
    Qc = _chk_q(Qidxs, cb.qdtype)
    num, den = cb.cols
    m, k, n = xc.shape[0], xc.shape[1], Qc.shape[0]
    _need(Qc.shape[1] * num == k * den,
          f"{what}: x has {k} columns but Qidxs {tuple(Qidxs.shape)} encodes {Qc.shape[1] * num // den}")
    _need(Qc.device == x.device, "Qidxs and x must be on the same device")
    return xc, Qc, m, n, k


def _product(op, cb, supported=None):
    """the op `op` (x (M, k) fp16 times the codes -> (M, n) fp16) on the entry point quip_<op>; supported = (shape
    predicate, what it needs)"""
    entry = _Entry("quip_" + op)

    def impl(x, Qidxs, *tables):
        tabs = cb.tables(x, *tables)
        xc, Qc, m, n, k = _operands(op, cb, x, Qidxs)
        _need(supported is None or supported[0](m, n, k), f"{op}: shape ({m}, {n}, {k}) needs {supported and supported[1]}")
        y = _empty((m, n), dtype=torch.float16, device=x.device)
        if y.numel():
            with torch.cuda.device(x.device):
                entry(xc.data_ptr(), Qc.data_ptr(), *_args(tabs), y.data_ptr(), m, n, k, _stream(x))
        return y
    return impl


_SKINNY = (e8p_mm_skinny_supported, "k % 128 == 0, n % 2 == 0")
_BATCHED = (lambda m, n, k: e8p_mm_batched_supported(max(m, 1), n, k), "k % 64 == 0 and n % 2 == 0")   # (any M >= 0)


def _decompress(name, cb):
    entry = _Entry(f"quip_decompress_{name}_origorder")

    def impl(Qidxs, *tables):
        tabs = cb.tables(Qidxs, *tables)
        Qc = _chk_q(Qidxs, cb.qdtype)
        k = Qc.shape[1] * cb.cols[0] // cb.cols[1]
        w = _empty((Qc.shape[0], k), dtype=torch.float16, device=Qidxs.device)
        with torch.cuda.device(Qidxs.device):
            entry(Qc.data_ptr(), *_args(tabs), w.data_ptr(), Qc.shape[0], k, _stream(Qidxs))
        return w
    return impl


def _e8p_mm_cuda(x, Qidxs, grid):
    """E8P12's product also takes 1 <= M < 32 on the matrix cores, through a workspace for the rows' digit planes"""
    (g,) = _CODEBOOKS["e8p"].tables(x, grid)
    xc, Qc, m, n, k = _operands("e8p_mm", _CODEBOOKS["e8p"], x, Qidxs)
    y = _empty((m, n), dtype=torch.float16, device=x.device)
    if y.numel() == 0:
        return y
    L = capi.lib()
    ws_bytes = L.quip_e8p_mm_workspace_bytes(m, n, k)
    ws = _empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    with torch.cuda.device(x.device):
        capi.check(L.quip_e8p_mm_origorder_ws(xc.data_ptr(), Qc.data_ptr(), g.data_ptr(), y.data_ptr(), m, n, k,
                                              _ptr(ws), ws_bytes, _stream(x)), "quip_e8p_mm_origorder_ws")
    return y


_IMPLS = {
    "hadamard": _hadamard_cuda,
    "had_transform": _had_transform_cuda,
    "had_transform_planes": _had_transform_planes_cuda,
    "e8p_gemv_planes": _e8p_gemv_planes_cuda,
    "e8p_gemv_planes_group": lambda planes, Qidxs, grid: _gemv(_GEMV_E8P, planes, Qidxs, grid),
    "d4_gemv_planes": lambda planes, Qidxs, grid: _gemv(_GEMV_D4, [planes], [Qidxs], grid)[0],
    "d4_gemv_planes_group": lambda planes, Qidxs, grid: _gemv(_GEMV_D4, planes, Qidxs, grid),
    "e8prvq3_gemv_planes_group": lambda planes, Qidxs, grid, e81b_i8: _gemv(_GEMV_RVQ3, planes, Qidxs, grid, e81b_i8),
    "rope_attn_decode": _rope_attn_decode_cuda,
    "ffn_engine": _ffn_engine_cuda,
    "block_engine": _block_engine_cuda,
    "rope_attn_decode_z": _rope_attn_decode_z_cuda,
    "e8p_gemv_fused": _e8p_gemv_fused_cuda,
    "had_transform_planes_group": _had_transform_planes_group_cuda,
    "had_chain_planes_group": _had_chain_planes_group_cuda,
    "had_transform_group": _had_transform_group_cuda,
    "e8p_mm_planes_rows": _e8p_mm_planes_rows_cuda,
    "had_transform_planes_rows": _had_transform_planes_rows_cuda,
    "e8p_gemv_planes_rows": lambda planes, Qidxs, grid: _gemv_rows(_GEMV_E8P, planes, Qidxs, grid),
    "e8p_quantize": _e8p_quantize_cuda,
    "argmax_step": _argmax_step_cuda,
    "gemv_planes_rows_mode": _gemv_planes_rows_mode_cuda,
    "had_transform_fused": _had_transform_fused_cuda,
    "had_transform_planes_fused": _had_transform_planes_fused_cuda,
}
for _cb_name, _cb in _CODEBOOKS.items():
    _IMPLS[f"{_cb_name}_mm_origorder"] = _product(f"{_cb_name}_mm_origorder", _cb)
    _IMPLS[f"{_cb_name}_mm_skinny"] = _product(f"{_cb_name}_mm_skinny", _cb, _SKINNY)
    _IMPLS[f"{_cb_name}_mm_batched"] = _product(f"{_cb_name}_mm_batched", _cb, _BATCHED)
    _IMPLS[f"decompress_{_cb_name}_origorder"] = _decompress(_cb_name, _cb)
_IMPLS["e8p_mm_origorder"] = _e8p_mm_cuda
for _name, _fn in _IMPLS.items():
    _lib.impl(_name, _fn, "CUDA")


# ---- fake (meta) implementations: shapes only, for torch.compile / export -----------------
def _reg_fake(name, fn):
    torch.library.register_fake("quip_lib::" + name, fn, lib=_lib)


_reg_fake("hadamard", lambda x, scale: torch.empty_like(x, memory_format=torch.contiguous_format))
_reg_fake("had_transform", lambda x, out_features, n, K, had, transpose, pre, pre2, post, bias, scale:
          x.new_empty((x.shape[0], out_features)))
_reg_fake("had_transform_planes", lambda x, n, K, had, transpose, pre, scale:
          x.new_empty((_planes_numel(n),), dtype=torch.uint8))
_reg_fake("had_transform_fused", lambda x, out_features, n, K, had, transpose, pre, pre2, post, bias, scale, residual,
          rms_weight, rms_eps, gate: x.new_empty((x.shape[0], out_features)))
_reg_fake("had_transform_planes_fused", lambda x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate,
          resid_scale=0.0: x.new_empty((_planes_numel(n, resid_scale),), dtype=torch.uint8))
_reg_fake("had_transform_planes_group", lambda x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate,
          resid_scale=0.0: [x.new_empty((_planes_numel(n, resid_scale),), dtype=torch.uint8) for _ in pre])
_reg_fake("had_chain_planes_group", lambda z, z_post, z_residual, z_scale, n, pre, scale, rms_weight, rms_eps,
          resid_scale=0.0, K=1, z_had=None, had=None:
          [z.new_empty((1, n))] + [z.new_empty((_planes_numel(n, resid_scale),), dtype=torch.uint8) for _ in pre])
_reg_fake("had_transform_group", lambda x, out_features, n, K, had, transpose, pre2, post, bias, scale, residual, pre,
          rms_weight, rms_eps, ns=None:
          [t.new_empty((t.shape[0], int(o))) for t, o in zip(x, out_features)])
_reg_fake("had_transform_planes_rows", lambda x, n, K, had, transpose, pre, scale, rms_weight, rms_eps, gate,
          resid_scale=0.0: x.new_empty((x.shape[0], _planes_numel(n, resid_scale)), dtype=torch.uint8))
_reg_fake("e8p_gemv_planes_rows", lambda planes, Qidxs, grid:
          Qidxs.new_empty((planes.shape[0], Qidxs.shape[0]), dtype=torch.float16))
_reg_fake("gemv_planes_rows_mode", lambda planes, Qidxs, grid, grid2, mode:
          Qidxs.new_empty((planes.shape[0], Qidxs.shape[0]), dtype=torch.float16))
_reg_fake("argmax_step", lambda logits, tok, pos: None)
_reg_fake("e8p_quantize", lambda X, grid: (torch.empty_like(X), X.new_empty((X.shape[0],), dtype=torch.int64)))
_reg_fake("e8p_mm_planes_rows", lambda planes, Qidxs, grid:
          Qidxs.new_empty((len(planes), Qidxs.shape[0]), dtype=torch.float16))
_reg_fake("e8p_gemv_fused", lambda x, z, post, residual, rms_weight, rms_eps, z_scale, pre, scale, Qidxs, grid:
          ([z.new_empty((1, z.numel()))] if z is not None else []) +
          [q.new_empty((1, q.shape[0]), dtype=torch.float16) for q in Qidxs])
_reg_fake("ffn_engine", lambda planes_gate, planes_up, q_gate, q_up, q_down, had3, sv_gate, sv_up, su_down, grid, workspace,
          out_scale, in_scale, K, dbg=None: q_down.new_empty((1, q_down.shape[0]), dtype=torch.float16))
_reg_fake("block_engine", lambda layers, h_in, pos, cos, sin, grid, workspace, n_layers, max_len, rms_eps, attn_scale,
          dbg=None, dbg_layer=-1, codebook=0, resid_scale=0.0, shape=0, grid2=None, kcache=None, vcache=None: torch.empty_like(h_in))
_reg_fake("rope_attn_decode", lambda q, k, v, cos, sin, pos, kcache, vcache, workspace=None, window=0: torch.empty_like(q))
_reg_fake("rope_attn_decode_z", lambda zs, posts, scales, cos, sin, pos, kcache, vcache, workspace=None, window=0:
          kcache.new_empty((zs[0].numel() // kcache.shape[2], kcache.shape[2])))
for _n in ("e8p_gemv_planes_group", "d4_gemv_planes_group", "e8prvq3_gemv_planes_group"):
    _reg_fake(_n, lambda planes, Qidxs, *tables: [q.new_empty((1, q.shape[0]), dtype=torch.float16) for q in Qidxs])
for _n in ("e8p_gemv_planes", "d4_gemv_planes"):
    _reg_fake(_n, lambda planes, Q, grid: Q.new_empty((1, Q.shape[0]), dtype=torch.float16))
for _cb_name, _cb in _CODEBOOKS.items():
    for _n in ("_mm_origorder", "_mm_skinny", "_mm_batched"):
        _reg_fake(_cb_name + _n, lambda x, Q, *tables: x.new_empty((x.shape[0], Q.shape[0]), dtype=torch.float16))
    _reg_fake(f"decompress_{_cb_name}_origorder", lambda Q, *tables, _c=_cb.cols:
              Q.new_empty((Q.shape[0], Q.shape[1] * _c[0] // _c[1]), dtype=torch.float16))


# ---- quantise-time: one LDLQ panel in one launch (csrc/quantize.hip) ------------------------------------
# Defined beside the table above like the ops of lora.py / score.py (_SCHEMAS is the reference's op surface plus the
# inference path's; tests/test_fakes_meta.py pins exactly that set).
LDLQ_PANEL_MAX_COLS = 128


def _ldlq_panel_cuda(A, B, M, P, grid):
    """A, B (m, c) fp32; M (c, c) fp32; P (c / 8, 8, 8) fp32 or None -> (hat (m, c) fp32, idx (m, c / 8) int64)"""
    _need(A.is_cuda and A.dim() == 2 and A.dtype == torch.float32 and A.is_contiguous(),
          "ldlq_panel: A must be a contiguous float32 (m, c) CUDA tensor")
    m, c = A.shape
    _need(c >= 8 and c % 8 == 0 and c <= LDLQ_PANEL_MAX_COLS,
          f"ldlq_panel: c = {c} (a multiple of 8 in 8 .. {LDLQ_PANEL_MAX_COLS})")
    _need(B.dtype == torch.float32 and B.is_contiguous() and B.device == A.device and tuple(B.shape) == (m, c),
          "ldlq_panel: B must be contiguous float32 with A's shape on A's device")
    _need(M.dtype == torch.float32 and M.is_contiguous() and M.device == A.device and tuple(M.shape) == (c, c),
          "ldlq_panel: M must be contiguous float32 (c, c) on A's device")
    _need(P is None or (P.dtype == torch.float32 and P.is_contiguous() and P.device == A.device
                        and tuple(P.shape) == (c // 8, 8, 8)),
          "ldlq_panel: P must be contiguous float32 (c / 8, 8, 8) on A's device, or None")
    g = _grid_i64(grid, A)
    hat = torch.empty_like(A)
    idx = _empty((m, c // 8), dtype=torch.int64, device=A.device)
    with torch.cuda.device(A.device):
        capi.check(capi.lib().quip_ldlq_panel_f32(A.data_ptr(), B.data_ptr(), M.data_ptr(), _ptr(P), m, c, g.data_ptr(),
                                                  hat.data_ptr(), idx.data_ptr(), _stream(A)), "quip_ldlq_panel_f32")
    return hat, idx


def _ldlq_panel_rvq_cuda(A, B, M, P, grid, resid_grid, resid_scale):
    """ldlq_panel with the two-stage step of the residual codebooks: resid_grid None -> E8P12RVQ4B (idx = a << 16 | b),
    the fp32 (256, 8) E81B entries -> E8P12RVQ3B (idx = a << 8 | b); hat = a + b * fp32(resid_scale)"""
    _need(A.is_cuda and A.dim() == 2 and A.dtype == torch.float32 and A.is_contiguous(),
          "ldlq_panel_rvq: A must be a contiguous float32 (m, c) CUDA tensor")
    m, c = A.shape
    _need(c >= 8 and c % 8 == 0 and c <= LDLQ_PANEL_MAX_COLS,
          f"ldlq_panel_rvq: c = {c} (a multiple of 8 in 8 .. {LDLQ_PANEL_MAX_COLS})")
    _need(B.dtype == torch.float32 and B.is_contiguous() and B.device == A.device and tuple(B.shape) == (m, c),
          "ldlq_panel_rvq: B must be contiguous float32 with A's shape on A's device")
    _need(M.dtype == torch.float32 and M.is_contiguous() and M.device == A.device and tuple(M.shape) == (c, c),
          "ldlq_panel_rvq: M must be contiguous float32 (c, c) on A's device")
    _need(P is None or (P.dtype == torch.float32 and P.is_contiguous() and P.device == A.device
                        and tuple(P.shape) == (c // 8, 8, 8)),
          "ldlq_panel_rvq: P must be contiguous float32 (c / 8, 8, 8) on A's device, or None")
    _need(resid_grid is None or (resid_grid.dtype == torch.float32 and resid_grid.is_contiguous()
                                 and resid_grid.device == A.device and tuple(resid_grid.shape) == (256, 8)),
          "ldlq_panel_rvq: resid_grid must be contiguous float32 (256, 8) on A's device, or None")
    s = float(resid_scale)
    _need(math.isfinite(s) and s != 0.0 and math.isfinite(ctypes.c_float(s).value) and ctypes.c_float(s).value != 0.0,
          f"ldlq_panel_rvq: resid_scale = {resid_scale} must be finite and non-zero in float32")
    g = _grid_i64(grid, A)
    hat = torch.empty_like(A)
    idx = _empty((m, c // 8), dtype=torch.int64, device=A.device)
    with torch.cuda.device(A.device):
        capi.check(capi.lib().quip_ldlq_panel_rvq_f32(A.data_ptr(), B.data_ptr(), M.data_ptr(), _ptr(P), m, c, g.data_ptr(),
                                                      _ptr(resid_grid), s, hat.data_ptr(), idx.data_ptr(), _stream(A)),
                   "quip_ldlq_panel_rvq_f32")
    return hat, idx


try:
    _lib.define("ldlq_panel_rvq(Tensor A, Tensor B, Tensor M, Tensor? P, Tensor grid, Tensor? resid_grid, "
                "float resid_scale) -> (Tensor hat, Tensor idx)")
    _lib.impl("ldlq_panel_rvq", _ldlq_panel_rvq_cuda, "CUDA")
    _reg_fake("ldlq_panel_rvq", lambda A, B, M, P, grid, resid_grid, resid_scale:
              (torch.empty_like(A), A.new_empty((A.shape[0], A.shape[1] // 8), dtype=torch.int64)))
except RuntimeError:
    pass

try:
    _lib.define("ldlq_panel(Tensor A, Tensor B, Tensor M, Tensor? P, Tensor grid) -> (Tensor, Tensor)")
    _lib.impl("ldlq_panel", _ldlq_panel_cuda, "CUDA")
    _reg_fake("ldlq_panel", lambda A, B, M, P, grid:
              (torch.empty_like(A), A.new_empty((A.shape[0], A.shape[1] // 8), dtype=torch.int64)))
except RuntimeError:
    pass
