"""quip_lib::block_engine_token: a whole greedy token in the persistent launch (csrc/token_tail.hip.h).

The launch reads `tok`, fetches its embedding row, runs the blocks and, behind the last one, applies the final RMSNorm,
multiplies lm_head, picks the arg-max and advances the position: `tok`, `pos`, `logits` and the workspace are mutated.
LlamaDecoder.step() takes it for greedy decoding on the 4096-wide shapes (decode.py); `QUIP_TOKEN_TAIL=0` keeps the
separate launches (embedding lookup, block_engine, rms_norm, lm_head product, argmax_step) for A/B."""
import ctypes

import torch

from . import capi
from . import register_lib as _R

try:
    _R._lib.define("block_engine_token(Tensor layers, Tensor(a!) tok, Tensor(b!) pos, Tensor embed, Tensor final_norm, "
                   "Tensor lm_head, Tensor(c!) logits, Tensor cos, Tensor sin, Tensor grid, Tensor(d!) workspace, "
                   "int n_layers, int max_len, float rms_eps, float attn_scale, Tensor? dbg=None, int dbg_layer=-1, "
                   "int codebook=0, float resid_scale=0.0, int shape=0, Tensor? grid2=None, "
                   # the KV caches the descriptors point into (as for block_engine), the debug output of the final norm
                   "Tensor(e!)? kcache=None, Tensor(f!)? vcache=None, Tensor(g!)? xnorm=None) -> ()")
except RuntimeError:
    pass


def _block_engine_token_cuda(layers, tok, pos, embed, final_norm, lm_head, logits, cos, sin, grid, workspace, n_layers,
                             max_len, rms_eps, attn_scale, dbg=None, dbg_layer=-1, codebook=0, resid_scale=0.0, shape=0,
                             grid2=None, kcache=None, vcache=None, xnorm=None):
    need = _R._need
    dev = lm_head.device
    lb = capi.lib().quip_block_engine_layer_bytes()
    need(layers.dtype == torch.uint8 and layers.is_contiguous() and layers.numel() >= n_layers * lb and layers.device == dev,
         "layers must be the packed descriptors (uint8, n_layers x 256 bytes) on the device")
    need(shape in (0, 2), "block_engine_token: shape 0 (hidden 4096, multi-head) or 2 (hidden 4096, grouped-query)")
    for t in (tok, pos):
        need(t.dtype == torch.int64 and t.numel() == 1 and t.device == dev, "tok / pos: int64 device scalars")
    need(lm_head.dtype == torch.float16 and lm_head.is_contiguous() and lm_head.dim() == 2 and lm_head.shape[1] == 4096,
         "lm_head: contiguous fp16 (vocab, 4096)")
    vocab = lm_head.shape[0]
    need(embed.dtype == torch.float16 and embed.is_contiguous() and tuple(embed.shape) == (vocab, 4096) and embed.device == dev,
         "embed: contiguous fp16 (vocab, 4096) on lm_head's device")
    need(final_norm.dtype == torch.float16 and final_norm.is_contiguous() and final_norm.numel() == 4096
         and final_norm.device == dev, "final_norm: fp16 [4096]")
    need(logits.dtype == torch.float16 and logits.is_contiguous() and logits.numel() == vocab and logits.device == dev,
         "logits: contiguous fp16 with vocab elements")
    if xnorm is not None:
        need(xnorm.dtype == torch.float16 and xnorm.is_contiguous() and xnorm.numel() == 4096 and xnorm.device == dev,
             "xnorm: fp16 [4096]")
    for t in (cos, sin):
        need(t.dtype == torch.float32 and t.is_contiguous() and t.shape == (max_len, 128) and t.device == dev,
             "cos / sin: fp32 [max_len, 128]")
    need(workspace.dtype == torch.uint8 and workspace.device == dev and workspace.numel() >= _R._block_engine_ws_bytes(shape),
         "workspace too small")
    if codebook in (1, 3):
        g = _R._d4_grid_f16(grid)
        need(g.device == dev and g.numel() == 1024, "D4 / HI grid: fp16 (256, 4) on the device")
    else:
        g = _R._grid_i64(grid, lm_head)
    if codebook == 4:
        need(grid2 is not None and grid2.dtype == torch.int8 and grid2.is_contiguous() and grid2.numel() == 2048
             and grid2.device == dev, "grid2: the E81B table as int8 (256, 8) on the device")
    a = capi.BlockEngineArgs(layers.data_ptr(), None, None, pos.data_ptr(), cos.data_ptr(), sin.data_ptr(), g.data_ptr(),
                             workspace.data_ptr(), _R._ptr(dbg), int(n_layers), int(max_len), int(dbg_layer), float(rms_eps),
                             float(attn_scale), int(codebook), float(resid_scale), int(shape),
                             _R._ptr(grid2) if codebook == 4 else None)
    t = capi.TokenTailArgs(tok.data_ptr(), pos.data_ptr(), embed.data_ptr(), final_norm.data_ptr(), lm_head.data_ptr(),
                           logits.data_ptr(), _R._ptr(xnorm), int(vocab))
    with torch.cuda.device(dev):
        capi.check(capi.lib().quip_block_engine_token(ctypes.byref(a), ctypes.byref(t), _R._stream(lm_head)),
                   "quip_block_engine_token")


try:
    _R._lib.impl("block_engine_token", _block_engine_token_cuda, "CUDA")
    _R._reg_fake("block_engine_token",
                 lambda layers, tok, pos, embed, final_norm, lm_head, logits, cos, sin, grid, workspace, n_layers, max_len,
                 rms_eps, attn_scale, dbg=None, dbg_layer=-1, codebook=0, resid_scale=0.0, shape=0, grid2=None, kcache=None,
                 vcache=None, xnorm=None: None)
except RuntimeError:
    pass
