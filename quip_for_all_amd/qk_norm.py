"""Per-head RMSNorm of q and k between the projections and the rotary embedding (Qwen3: self_attn.q_norm / k_norm).

quip_lib::qk_norm_rows normalises every head of q (rows, heads * hd) and k (rows, kv_heads * hd) in place, one launch
(csrc/qk_norm.hip.h); quip_lib::rope_attn_decode_qknorm / rope_attn_decode_batched_qknorm are the bs = 1 and the
contiguous batched decode launches with the norm applied to q and to the new k row in registers -- bit for bit
qk_norm_rows followed by the plain launch, in the output and in the appended cache row.

The arithmetic (csrc/attn_query.hip.h), for one head vector x (fp16), weight w (fp16), eps (fp32):
    S = sum x_i^2 (fp32),  r = 1 / sqrt(S / hd + eps) (fp32),  n_i = fp16(x_i r),  y_i = fp16(float(n_i) float(w_i))
-- HF's Qwen3RMSNorm.forward.  `qk_norm_ref` is its float64 statement with an interval for r."""
import math

import numpy as np
import torch

from . import capi
from . import register_lib as _R

try:
    _R._lib.define("qk_norm_rows(Tensor(a!) q, Tensor(b!) k, Tensor q_weight, Tensor k_weight, int head_dim, float eps) -> ()")
    _R._lib.define("rope_attn_decode_qknorm(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, "
                   "Tensor(a!) kcache, Tensor(b!) vcache, Tensor(c!)? workspace, int window, Tensor q_weight, "
                   "Tensor k_weight, float eps) -> Tensor")
    _R._lib.define("rope_attn_decode_batched_qknorm(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, "
                   "Tensor(a!) kcache, Tensor(b!) vcache, Tensor(c!)? workspace, int window, Tensor q_weight, "
                   "Tensor k_weight, float eps) -> Tensor")
except RuntimeError:
    pass


def _check_weights(what, q, hd, q_weight, k_weight):
    for w in (q_weight, k_weight):
        _R._need(w.dtype == torch.float16 and w.is_contiguous() and w.device == q.device and tuple(w.shape) == (hd,),
                 f"{what}: q_weight / k_weight must be contiguous float16 (head_dim,) on q's device")


def _qk_norm_rows_cuda(q, k, q_weight, k_weight, head_dim, eps):
    """q (rows, heads * hd), k (rows, kv_heads * hd) fp16 contiguous, normalised in place"""
    need = _R._need
    hd = int(head_dim)
    need(hd in (64, 128), f"qk_norm_rows: head_dim {hd} (64 or 128)")
    for t in (q, k):
        need(t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.is_contiguous() and t.device == q.device,
             "qk_norm_rows: q / k must be contiguous float16 (rows, width) on one CUDA device")
    need(q.shape[0] == k.shape[0] and q.shape[0] >= 1, "qk_norm_rows: q and k need the same number of rows (>= 1)")
    need(q.shape[1] >= hd and k.shape[1] >= hd and q.shape[1] % hd == 0 and k.shape[1] % hd == 0,
         "qk_norm_rows: the widths of q and k must be multiples of head_dim")
    _check_weights("qk_norm_rows", q, hd, q_weight, k_weight)
    with torch.cuda.device(q.device):
        capi.check(capi.lib().quip_qk_norm_rows_f16(q.data_ptr(), k.data_ptr(), q_weight.data_ptr(), k_weight.data_ptr(),
                                                    q.shape[0], q.shape[1] // hd, k.shape[1] // hd, hd, float(eps),
                                                    _R._stream(q)), "quip_qk_norm_rows_f16")


def _rope_attn_decode_qknorm_cuda(q, k, v, cos, sin, pos, kcache, vcache, workspace, window, q_weight, k_weight, eps):
    """quip_lib::rope_attn_decode with the norm on q and the new k row"""
    _, heads, kvh, hd, max_len, _ = _R._check_attn("rope_attn_decode", "bs1", q, k, v, cos, sin, pos, kcache, vcache)
    _R._check_attn_workspace(workspace, q, None, heads, hd)
    _check_weights("rope_attn_decode_qknorm", q, hd, q_weight, k_weight)
    out = torch.empty_like(q)
    _R._attn_call("quip_rope_attn_decode_qknorm_f16", q, *_R._ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), heads, kvh, hd,
                  max_len, 1.0 / math.sqrt(hd), int(window), _R._ptr(workspace), _R._stream(q), q_weight.data_ptr(),
                  k_weight.data_ptr(), float(eps))
    return out


def _rope_attn_decode_batched_qknorm_cuda(q, k, v, cos, sin, pos, kcache, vcache, workspace, window, q_weight, k_weight,
                                          eps):
    """quip_lib::rope_attn_decode_batched with the norm on q and the new k rows"""
    B, heads, kvh, hd, max_len, _ = _R._check_attn("rope_attn_decode_batched", "batched", q, k, v, cos, sin, pos, kcache, vcache)
    _R._check_attn_workspace(workspace, q, B, heads, hd)
    _check_weights("rope_attn_decode_batched_qknorm", q, hd, q_weight, k_weight)
    out = torch.empty_like(q)
    _R._attn_call("quip_rope_attn_decode_batched_qknorm_f16", q, *_R._ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), B, heads,
                  kvh, hd, max_len, 1.0 / math.sqrt(hd), int(window), _R._ptr(workspace), _R._stream(q), q_weight.data_ptr(),
                  k_weight.data_ptr(), float(eps))
    return out


try:
    _R._lib.impl("qk_norm_rows", _qk_norm_rows_cuda, "CUDA")
    _R._lib.impl("rope_attn_decode_qknorm", _rope_attn_decode_qknorm_cuda, "CUDA")
    _R._lib.impl("rope_attn_decode_batched_qknorm", _rope_attn_decode_batched_qknorm_cuda, "CUDA")
    _R._reg_fake("qk_norm_rows", lambda q, k, q_weight, k_weight, head_dim, eps: None)
    _R._reg_fake("rope_attn_decode_qknorm", lambda q, k, v, cos, sin, pos, kcache, vcache, workspace, window, q_weight,
                 k_weight, eps: torch.empty_like(q))
    _R._reg_fake("rope_attn_decode_batched_qknorm", lambda q, k, v, cos, sin, pos, kcache, vcache, workspace, window,
                 q_weight, k_weight, eps: torch.empty_like(q))
except RuntimeError:
    pass


def qk_norm_ref(x, w, eps, rel=2.0 ** -19):
    """The norm of the module docstring in float64 with r (1 -+ rel) for r: x (..., hd) fp16 head vectors, w (hd,) fp16,
    eps taken as the fp32 value the kernels get -> (lo, hi), the per-element fp16 interval of y (fp16 CPU tensors of x's
    shape; y is monotone in r, so the two ends of r give the two ends of y).  rel = 2^-19 covers any order of the hd
    positive additions, the sqrt and the divide in fp32 and the fp32 product x r: about 15 roundings of 2^-24."""
    x64 = np.asarray(x.detach().cpu().to(torch.float16).numpy(), dtype=np.float64)
    w64 = np.asarray(w.detach().cpu().to(torch.float16).numpy(), dtype=np.float64)
    hd = x64.shape[-1]
    eps = float(np.float32(eps))
    with np.errstate(all="ignore"):
        r = 1.0 / np.sqrt((x64 * x64).sum(-1, keepdims=True) / hd + eps)
        ends = []
        for f in (1.0 - rel, 1.0 + rel):
            n = (x64 * (r * f)).astype(np.float16)                 # (numpy rounds float64 -> float16 in one step)
            ends.append((n.astype(np.float64) * w64).astype(np.float16))
    lo = np.minimum(ends[0], ends[1])
    hi = np.maximum(ends[0], ends[1])
    return torch.from_numpy(lo), torch.from_numpy(hi)
