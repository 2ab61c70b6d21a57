"""bs=1 greedy decode harness for Llama-architecture models whose linear layers are
QuantLinear (the metric driver of the reference, example_generate.py:9-59,62-110:
static KV cache + one captured single-token step, sampling on the device).

The reference relies on HF `StaticCache` + `torch.compile(mode="reduce-overhead")`;
`_setup_cache` is a transformers-4.38 API that no longer exists, and there is no tracing
compiler in this stack by design, so the step is written once with static shapes and
captured in a hipGraph (torch.cuda.CUDAGraph): one graph replay per token, no host sync
inside the loop (the next token id stays on the device).

Only the linear layers are the QuIP# hot path; embeddings, norms, RoPE, attention over the
cache and the fp16 lm_head use stock torch ops (they are what remains once the GEMVs are
fast: SURVEY.md 8f rank 1)."""
import math
import os
import warnings
import weakref
from contextlib import contextmanager
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

from . import chunk_attn as _chunk_attn  # noqa: F401  (defines quip_lib::rope_attn_chunk)
from . import lora as _lora  # (defines quip_lib::lora_shrink_rows / lora_expand_rows)
from . import qk_norm as _qk_norm  # noqa: F401  (defines quip_lib::qk_norm_rows and the two _qknorm decode launches)
from . import register_lib as _R
from . import score as _score  # (defines quip_lib::nll_rows)
from . import spec as _spec  # (defines quip_lib::spec_draft / spec_accept_draft)
from . import token_tail as _token_tail  # noqa: F401  (defines quip_lib::block_engine_token)
from .codebook import codebook_id
from .qlinear import (QuantLinear, _engine_had3, chain_planes, chain_supported, ffn_engine, ffn_engine_ok, forward_group,
                      fused_in_supported, gemv_chain, gemv_fused, gemv_group_unfused, gemv_unfused, out_transform_group)

PROJECTIONS = ("q", "k", "v", "o", "gate", "up", "down")      # the seven QuantLinear modules of a decoder block
_ENGINE_CODEBOOK_TILED = 5     # E8P12 on launch-tiled copies of the codes (shape 0: LlamaDecoder._init_block_engine)
_ENGINE_CODEBOOK = {"E8P12": 0, "D4": 1, "E8P12RVQ4B": 2, "HI": 3, "E8P12RVQ3B": 4}     # the persistent launch's table modes


@dataclass
class LlamaShape:
    hidden: int = 4096
    ffn: int = 11008
    layers: int = 32
    heads: int = 32
    kv_heads: int = 32
    vocab: int = 32000
    rms_eps: float = 1e-5
    rope_theta: float = 10000.0
    head_dim: int = None      # unset: hidden // heads; Qwen3 sets its own (q and o are heads * head_dim wide, not hidden)

    def __post_init__(self):
        if self.head_dim is None:
            self.head_dim = self.hidden // self.heads

    @property
    def q_width(self):
        """width of q_proj's output, of the attention output and of o_proj's input"""
        return self.heads * self.head_dim


LLAMA2_7B = LlamaShape()
LLAMA2_70B = LlamaShape(hidden=8192, ffn=28672, layers=80, heads=64, kv_heads=8)
LLAMA3_8B = LlamaShape(hidden=4096, ffn=14336, layers=32, heads=32, kv_heads=8, vocab=128256)   # also Mistral-7B's block (vocab 32000)
SMALL = LlamaShape(hidden=1024, ffn=2816, layers=2, heads=8, kv_heads=4, vocab=1024)   # takes the fused-prologue path
TINY = LlamaShape(hidden=256, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512)


def random_quant_linear(in_f, out_f, codebook="E8P12", generator=None, device="cuda", **cb_kwargs):
    """QuantLinear with uniformly random codes (every code is a valid lattice point), +-1 SU/SV,
    random orthogonal had factors and a scale that keeps |y| ~ |x| (random-init analogue of a
    quantised checkpoint)."""
    cb = codebook_id[codebook](inference=True, **cb_kwargs)
    layer = QuantLinear(in_f, out_f, cb, bias=False, use_rand=True)
    g = generator
    dev = torch.device(device)
    on_dev = g is not None and g.device.type == dev.type == "cuda"   # large models: draw the codes on the GPU
    gdev = dev if on_dev else "cpu"
    with torch.no_grad():
        q = layer.Qidxs
        if q.dtype == torch.int16:
            codes = torch.randint(-32768, 32768, q.shape, generator=g, dtype=torch.int32, device=gdev).to(torch.int16)
        elif q.dtype == torch.uint8:
            codes = torch.randint(0, 256, q.shape, generator=g, dtype=torch.int32, device=gdev).to(torch.uint8)
        else:
            codes = torch.randint(-2 ** 31, 2 ** 31 - 1, q.shape, generator=g, dtype=torch.int64,
                                  device=gdev).to(torch.int32)
        su = (torch.randint(0, 2, (in_f,), generator=g, device=gdev) * 2 - 1).to(torch.float16)
        sv = (torch.randint(0, 2, (out_f,), generator=g, device=gdev) * 2 - 1).to(torch.float16)
        if on_dev:
            layer = layer.to(dev)
        layer.Qidxs.copy_(codes)
        layer.SU.copy_(su)
        layer.SV.copy_(sv)
        wrms = {"E8P12": 1.03, "E8P12RVQ3B": 1.2, "E8P12RVQ4B": 1.2, "D4": 1.21, "HI": 4.6}[codebook]
        layer.Wscale.fill_(1.0 / (wrms * math.sqrt(in_f)))
    layer.wscale_float = float(layer.Wscale)      # quantizer.py:836-837
    return layer.to(device).eval()


def tile_codes(qidxs):
    """The persistent 8192-wide launch's layout of a code matrix (include/quip_mi355.h: quip_tile_codes; decode_block_gqa.hip):
    inside every aligned block of 16 rows the 64-byte pieces of the 16 rows lie side by side, piece after piece --
    tiled[rb][c][q][n] = bytes [64 c + 16 q, +16) of row 16 rb + n -- so that one load instruction of the product (16 rows x
    64 bytes in the checkpoint's layout; origin_order.cu:388-555 walks it row-major) covers 1 KB of consecutive bytes.
    Returns a flat uint8 tensor of the same size on the same device."""
    from . import capi
    b = qidxs.detach().contiguous().view(torch.uint8).reshape(qidxs.shape[0], -1)
    rows, rb = b.shape
    out = torch.empty(rows * rb, dtype=torch.uint8, device=b.device)
    if not b.is_cuda:
        raise capi.QuipNativeError("tile_codes: the codes must be on the GPU (there is no CPU path)")
    with torch.cuda.device(b.device):
        capi.check(capi.lib().quip_tile_codes(b.data_ptr(), out.data_ptr(), rows, rb, torch.cuda.current_stream(b.device).cuda_stream),
                   "quip_tile_codes")
    return out


def untile_codes(tiled, rows, row_bytes, out):
    """the inverse of tile_codes (quip_untile_codes): `tiled` (flat uint8) -> the row-major matrix, written into `out` (any dtype,
    rows * row_bytes bytes)"""
    from . import capi
    with torch.cuda.device(tiled.device):
        capi.check(capi.lib().quip_untile_codes(tiled.data_ptr(), out.data_ptr(), rows, row_bytes,
                                                torch.cuda.current_stream(tiled.device).cuda_stream), "quip_untile_codes")
    return out


def tile_codes_view(qidxs, inverse=False):
    """The shape-0 launch's layout of a gate / up matrix (include/quip_mi355.h: quip_tile_codes_view; decode_block_tiled.hip): the
    (K, 256) view of its rows -- rows k * 256 + j -- column by column, each column in blocks of 16 view rows with the last one short
    and no padding: view[j][b][c][q][n < nb(b)] = bytes [64 c + 16 q, +16) of row (16 b + n) * 256 + j.  `qidxs`: the (rows, ...)
    matrix on the GPU -> a flat uint8 tensor of the same size; inverse=True: the tiled bytes (given with the matrix's 2-D shape)
    -> the row-major bytes."""
    from . import capi
    b = qidxs.detach().contiguous().view(torch.uint8).reshape(qidxs.shape[0], -1)
    rows, rb = b.shape
    if not b.is_cuda:
        raise capi.QuipNativeError("tile_codes_view: the codes must be on the GPU (there is no CPU path)")
    out = torch.empty(rows * rb, dtype=torch.uint8, device=b.device)
    fn = capi.lib().quip_untile_codes_view if inverse else capi.lib().quip_tile_codes_view
    with torch.cuda.device(b.device):
        capi.check(fn(b.data_ptr(), out.data_ptr(), rows, rb, torch.cuda.current_stream(b.device).cuda_stream),
                   "quip_untile_codes_view" if inverse else "quip_tile_codes_view")
    return out


def _launch_tiled_codes(L):
    """shape 0 with E8P12: the seven code matrices of block L in the launch's own layout (decode_block_tiled.hip: every weight
    request one run of consecutive bytes) -- one more copy of the codes in HBM (+1.63 GB for Llama-2-7B), made once per model and
    again by every rebuild of the descriptors; the modules' `Qidxs` stay what everything else reads"""
    return [tile_codes_view(L[k].Qidxs) if k in ("gate", "up") else tile_codes(L[k].Qidxs) for k in PROJECTIONS]


def qidxs_nbytes(m):
    """bytes of a module's code matrix (its row-major tensor, or -- LlamaDecoder(single_copy=True) -- the tiled copy that replaced it)"""
    return m.Qidxs.numel() * m.Qidxs.element_size() if m.Qidxs is not None else m._qidxs_tiled.numel()


# ---- what the persistent block launch reads of one decoder block (LlamaDecoder._init_block_engine) -----------------------------
def _f16(t):
    return t.detach().to(torch.float16).contiguous()


def _strided(t, per_thread):
    """a vector in the strided layout of the launch's 512-thread transforms: p[per_thread t + k] = v[t + 512 k]"""
    return _f16(t).reshape(per_thread, 512).t().contiguous().reshape(-1)


def _engine_vectors(L, per_thread):
    """(SU x 7, SV x 7, [ln1, ln2]) of block L.  The vectors the launch multiplies inside a strided transform -- ln, SU of
    q k v gate up, SV of o and down -- are pre-permuted: 16 elements per thread on the 8192-wide shape, 8 on the 4096-wide ones"""
    su = [_f16(L[k].SU) if k in ("o", "down") else _strided(L[k].SU, per_thread) for k in PROJECTIONS]
    sv = [_strided(L[k].SV, per_thread) if k in ("o", "down") else _f16(L[k].SV) for k in PROJECTIONS]
    return su, sv, [_strided(L["ln1"], per_thread), _strided(L["ln2"], per_thread)]


def _had3_mix(L, dev):
    """shape 1: the K x K factors of gate, up (right) and down (left, transposed) as fp32 rows of 8"""
    K = L["gate"].K_right
    mix = torch.zeros(3, K, 8, dtype=torch.float32, device=dev)
    mix[0, :, :K] = L["gate"].had_right.detach().float()
    mix[1, :, :K] = L["up"].had_right.detach().float()
    mix[2, :, :K] = L["down"].had_left.detach().float().t()
    return mix.contiguous()


def _had3_k56(L, dev):
    """shape 2 (Llama-3-8B / Mistral-7B, n_ffn = 14336 = 56 x 256):
    (R_7 (x) H_2048) / sqrt 2048 on the (7, 2048) view = ((R_7 (x) H_8) (x) H_256) / (sqrt 8 sqrt 256) on the (56, 256) view:
    the launch's K = 56 factors are R_7 (x) H_8 (entries +-R_7: exact in fp16); it folds the 1 / sqrt 8 into its scales
    (decode_block.hip: kMixScale; the descriptor's scale of down is wscale / sqrt 2048 already)"""
    h8 = torch.tensor([[1.0 - 2.0 * (bin(i & j).count("1") & 1) for j in range(8)] for i in range(8)], device=dev)
    k56 = lambda r: torch.kron(r.detach().float(), h8)      # noqa: E731
    had3 = torch.zeros(2 * 3136 + 64 * 72, dtype=torch.float16, device=dev)      # (down's: rows of 72: bank spread)
    had3[:3136] = k56(L["gate"].had_right).to(torch.float16).reshape(-1)
    had3[3136:6272] = k56(L["up"].had_right).to(torch.float16).reshape(-1)
    hdT = torch.zeros(64, 72, dtype=torch.float16, device=dev)
    hdT[:56, :56] = k56(L["down"].had_left).to(torch.float16).T
    had3[6272:] = hdT.reshape(-1)
    return had3


def _tiled_codes(mods, single_copy):
    """shape 1 streams a re-tiled copy of the codes (decode_block_gqa.hip: full-line requests): one more copy of the weights in
    HBM, made once per model; the checkpoint's tensors stay what the stage-wise step and prefill read -- unless `single_copy`:
    then the tiled copy replaces the module's `Qidxs` (its shape and dtype are kept for LlamaDecoder._row_major).  A tiled copy
    that exists is the truth and is used as it is: `Qidxs` may be None, or scratch lent by _row_major.  So the codes of a
    single-copy module cannot be replaced after the build (load_state_dict into `Qidxs`): the tiled copy would stay."""
    wq = []
    for m in mods:
        t = getattr(m, "_qidxs_tiled", None)
        if t is None:
            t = tile_codes(m.Qidxs)
            if single_copy:
                m._qidxs_meta = (tuple(m.Qidxs.shape), m.Qidxs.dtype)
                m._qidxs_tiled, m.Qidxs = t, None
        wq.append(t)
    return wq


def capture_graph(warmup, body):
    """warmup() on a side stream (kernel attribute setup, allocator), then body() captured as a hipGraph, synchronised after
    each -> (graph, what body() returned: the static outputs, valid after every replay)"""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        warmup()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        out = body()
    torch.cuda.synchronize()
    return graph, out


def _extend_chunks(dec, what, tokens, chunk, kv, pos, on_chunk, adapter=None):
    """the chunk loop of extend() / score(): `tokens` behind the position in chunks of at most `chunk` rows, every block
    over each chunk, the position advanced on the device; on_chunk(c0, h) gets the hidden rows h (n, hidden) of the
    chunk that starts at token c0.  `adapter`: the (1,) int32 adapter index of the sequence (enable_lora; default: the
    bs = 1 decoder's), spread over each chunk's rows on the device"""
    s = dec.s
    tokens = torch.as_tensor(tokens, dtype=torch.long, device=dec.dev).reshape(-1)
    P, chunk = tokens.numel(), int(chunk)
    if P < 1:
        raise ValueError(f"{what}: an empty token list")
    if chunk < 1:
        raise ValueError(f"{what}: chunk {chunk} < 1")
    if s.head_dim not in (64, 128):
        raise NotImplementedError(f"head_dim {s.head_dim}: the chunk attention launch serves 64 and 128")
    kcache, vcache = (dec.kcache, dec.vcache) if kv is None else kv
    pos = dec.pos if pos is None else pos

    def attend(i, q, k, v):
        n, kc, vc = q.shape[0], kcache[i], vcache[i]
        return torch.ops.quip_lib.rope_attn_chunk(
            q.view(n, s.heads, s.head_dim), k.view(n, s.kv_heads, s.head_dim), v.view(n, s.kv_heads, s.head_dim),
            dec.cos[:kc.shape[1]], dec.sin[:kc.shape[1]], pos, kc, vc, dec.window).reshape(n, s.q_width)
    for c0 in range(0, P, chunk):
        n = min(chunk, P - c0)
        h = dec.embed[tokens[c0:c0 + n]]                           # (n, hidden)
        rows_adapter = dec._rows_adapter(adapter, n)
        for i, L in enumerate(dec.layers):
            h = dec._block(L, h, partial(attend, i), adapter=rows_adapter)
        pos.add_(n)
        on_chunk(c0, h)


class LlamaDecoder:
    """Random-init Llama with QuantLinear projections, static KV cache, bs=1.

    single_copy (or QUIP_SINGLE_COPY=1; the 8192-wide persistent launch only -- it streams a RE-TILED copy of the codes,
    tile_codes()): keep ONE copy of the code matrices.  The modules' row-major `Qidxs` are dropped (set to None: every operator that
    would read them fails loudly, and `state_dict()` no longer holds them -- a decode-only serving mode, not one to save checkpoints
    from) once the tiled copies exist; the prompt pass and the stage-wise fallback get a matrix back in the checkpoint's layout,
    one decoder block at a time, in scratch buffers (untile_codes: 2 x 214 MB of traffic per block at HBM speed).  Llama-2-70B
    E8P12: 17.1 GB of codes resident instead of 34.2 GB."""

    def __init__(self, shape: LlamaShape = LLAMA2_7B, codebook="E8P12", max_len=256, device="cuda", seed=0,
                 device_init=False, window=0, single_copy=None, qk_norm=False, **cb_kwargs):
        if single_copy is None:
            single_copy = bool(int(os.environ.get("QUIP_SINGLE_COPY", "0")))
        self.s, self.dev, self.max_len = shape, torch.device(device), max_len
        g = torch.Generator().manual_seed(seed)
        gq = torch.Generator(device=self.dev).manual_seed(seed) if device_init else g
        s = shape
        kv = s.kv_heads * s.head_dim

        def ql(i, o):
            return random_quant_linear(i, o, codebook, gq, device, **cb_kwargs)

        def vec(n):
            return (1.0 + 0.02 * torch.randn(n, generator=g)).to(torch.float16).to(self.dev)

        self.embed = (0.5 * torch.randn(s.vocab, s.hidden, generator=g)).to(torch.float16).to(self.dev)
        self.lm_head = (torch.randn(s.vocab, s.hidden, generator=g) / math.sqrt(s.hidden)).to(torch.float16).to(self.dev)
        self.final_norm = vec(s.hidden)
        self.layers = []
        for _ in range(s.layers):
            self.layers.append(dict(
                ln1=vec(s.hidden), ln2=vec(s.hidden),
                q=ql(s.hidden, s.q_width), k=ql(s.hidden, kv), v=ql(s.hidden, kv), o=ql(s.q_width, s.hidden),
                gate=ql(s.hidden, s.ffn), up=ql(s.hidden, s.ffn), down=ql(s.ffn, s.hidden)))
            if qk_norm:
                # per-head RMSNorm of q and k in front of the rotation (Qwen3); drawn behind the block's other parameters,
                # and only then: without the flag the random stream is untouched
                for name in ("q_norm", "k_norm"):
                    self.layers[-1][name] = (1.0 + 0.1 * torch.randn(s.head_dim, generator=g)).to(torch.float16).to(self.dev)
        self.qk_eps = float(s.rms_eps)
        # (sliding-window attention, HF config.sliding_window: a window that covers the whole cache is full attention)
        self._init_runtime(window=int(window) if 0 < int(window) < max_len else 0, single_copy=single_copy)

    # architectures whose decoder block is Llama's: RMSNorm (weight only) -> q / k / v (+ bias) -> rotary -> softmax attention
    # -> o -> residual -> RMSNorm -> SiLU-gated MLP -> residual, embeddings and residuals unscaled
    LLAMA_LIKE = ("llama", "mistral", "qwen2", "qwen3")

    @classmethod
    def from_hf(cls, model, max_len=256, device=None, assume_llama_like=False, kv_cache=None):
        """Fast bs=1 decoder around a Llama-architecture HF model whose linear layers are QuantLinear
        (what `load_quantized_model` returns): shares the modules / weights, adds the static KV cache and
        the captured step.  Needs `model.model.{embed_tokens, layers, norm}` and `model.lm_head`.
        `kv_cache` = (keys, values): per-layer fp16 tensors (kv_heads, max_len, head_dim) to use as the static cache instead of
        allocating one (hf_fast.py binds the tensors of a transformers StaticCache this way; bind_kv() swaps them later).
        Architectures outside LLAMA_LIKE are refused (Gemma scales embeddings and norms, StableLM uses LayerNorm, ...:
        the module names match, the arithmetic does not) unless `assume_llama_like` vouches for them; such checkpoints run
        through `load_quantized_model` + the stock HF `generate`.  `config.head_dim` is free (Qwen3: heads * head_dim need not be
        hidden_size), and a `self_attn.q_norm` / `k_norm` pair that is an RMSNorm over head_dim is taken (_hf_qk_norm)."""
        cfg = model.config
        dev = torch.device(device) if device is not None else next(model.parameters()).device
        self = cls.__new__(cls)
        mt = getattr(cfg, "model_type", "")
        if mt not in cls.LLAMA_LIKE and not assume_llama_like:
            raise NotImplementedError(f"model_type {mt!r}: only {cls.LLAMA_LIKE} are known to have Llama's decoder block "
                                      "(pass assume_llama_like=True if this one does)")
        if getattr(cfg, "hidden_act", "silu") != "silu":
            raise NotImplementedError(f"hidden_act {cfg.hidden_act!r}: the MLP here is SiLU-gated")
        # the normalisation must be y = x / sqrt(mean(x^2) + eps) * weight: checked on numbers, not on a class name
        n0 = model.model.layers[0].input_layernorm
        with torch.no_grad():
            xt = torch.linspace(-2.0, 3.0, cfg.hidden_size, dtype=torch.float32, device=n0.weight.device)[None]
            want = xt / torch.sqrt((xt * xt).mean() + cfg.rms_norm_eps) * n0.weight.float()
            got = n0(xt.to(n0.weight.dtype)).float()
        if getattr(n0, "bias", None) is not None or not torch.allclose(got, want, rtol=2e-2, atol=2e-2):
            raise NotImplementedError(f"{type(n0).__name__} is not RMSNorm(x) * weight with eps = rms_norm_eps")
        heads = cfg.num_attention_heads
        rope = getattr(cfg, "rope_theta", None)
        rp = getattr(cfg, "rope_parameters", None) or getattr(cfg, "rope_scaling", None) or {}
        if rope is None:
            rope = rp.get("rope_theta", 10000.0) if isinstance(rp, dict) else 10000.0
        # what this decoder does not implement must not pass silently (the HF forward of the same model would differ)
        head_dim = getattr(cfg, "head_dim", None) or cfg.hidden_size // heads      # (free: Qwen3-0.6B has 1024 / 16 heads of 128)
        # q / k norms over head_dim (Qwen3) are taken, on any accepted architecture; any other norm there is refused
        qk_norms = [cls._hf_qk_norm(blk.self_attn, head_dim) for blk in model.model.layers]
        if any(n is None for n in qk_norms) and not all(n is None for n in qk_norms):
            raise NotImplementedError("q_norm / k_norm on some blocks only")
        if qk_norms[0] is not None and len({n[2] for n in qk_norms}) != 1:
            raise NotImplementedError("q_norm / k_norm with different eps per block")
        prf = rp.get("partial_rotary_factor", None) if isinstance(rp, dict) else None
        prf = getattr(cfg, "partial_rotary_factor", prf)
        if prf not in (None, 1, 1.0):
            raise NotImplementedError(f"partial rotary embeddings (factor {prf}) are not supported")
        window = 0
        # (HF's Llama modelling code never reads `sliding_window`: on such a config the attribute changes nothing there,
        #  so it changes nothing here)
        if (getattr(cfg, "sliding_window", None) and getattr(cfg, "use_sliding_window", True)
                and getattr(cfg, "model_type", "") != "llama"):
            types = getattr(cfg, "layer_types", None)
            if not types:
                # older Qwen2-style configs have no layer_types: HF applies the window to layers >= max_window_layers only
                # (modeling_qwen2.py), so the per-layer pattern follows from that field
                mwl = getattr(cfg, "max_window_layers", None)
                nl = cfg.num_hidden_layers
                types = ["sliding_attention"] if mwl is None else \
                    ["full_attention" if i < int(mwl) else "sliding_attention" for i in range(nl)]
            if any(t not in ("full_attention", "sliding_attention") for t in types) or len(set(types)) > 1:
                raise NotImplementedError(f"layer_types {sorted(set(types))}: per-layer attention patterns are not supported")
            # a window that is never shorter than the context is full attention (Mistral-7B: 4096 on a 4096 cache); a
            # shorter one bounds the attention walk from below -- the cache stays linear (row t = position t)
            if types[0] == "sliding_attention" and max_len > int(cfg.sliding_window):
                window = int(cfg.sliding_window)
        # rotary frequencies and attention scaling as the model computes them (llama3 / linear / yarn scaling change
        # inv_freq at every position; taking only rope_theta from the config would silently give other logits)
        inv_freq, att_scale = None, 1.0
        rot = getattr(model.model, "rotary_emb", None)
        if rot is not None and hasattr(rot, "inv_freq"):
            rope_type = getattr(rot, "rope_type", None) or (rp.get("rope_type", "default") if isinstance(rp, dict) else "default")
            if rope_type in ("dynamic", "longrope"):
                raise NotImplementedError(f"rope_type {rope_type!r}: frequencies depend on the sequence length")
            inv = rot.inv_freq.detach().to(torch.float32).cpu()
            if inv.numel() != head_dim // 2:
                raise NotImplementedError(f"rotary_emb.inv_freq has {inv.numel()} entries for head_dim {head_dim}")
            inv_freq, att_scale = inv, float(getattr(rot, "attention_scaling", 1.0) or 1.0)
        self.s = LlamaShape(hidden=cfg.hidden_size, ffn=cfg.intermediate_size, layers=cfg.num_hidden_layers,
                            heads=heads, kv_heads=getattr(cfg, "num_key_value_heads", heads) or heads,
                            vocab=cfg.vocab_size, rms_eps=cfg.rms_norm_eps, rope_theta=float(rope), head_dim=int(head_dim))
        self.dev, self.max_len = dev, max_len
        h16 = lambda t: t.detach().to(device=dev, dtype=torch.float16).contiguous()  # noqa: E731
        self.embed = h16(model.model.embed_tokens.weight)
        self.lm_head = h16(model.lm_head.weight)
        self.final_norm = h16(model.model.norm.weight)
        self.layers = []
        self.qk_eps = float(cfg.rms_norm_eps)
        for blk, norms in zip(model.model.layers, qk_norms):
            a, m = blk.self_attn, blk.mlp
            mods = dict(q=a.q_proj, k=a.k_proj, v=a.v_proj, o=a.o_proj, gate=m.gate_proj, up=m.up_proj, down=m.down_proj)
            for name, mod in mods.items():
                if not isinstance(mod, QuantLinear):
                    raise TypeError(f"{name}_proj is {type(mod).__name__}, expected QuantLinear")
                mod.to(dev).eval()
            self.layers.append(dict(ln1=h16(blk.input_layernorm.weight), ln2=h16(blk.post_attention_layernorm.weight),
                                    **mods))
            if norms is not None:
                self.layers[-1]["q_norm"], self.layers[-1]["k_norm"] = h16(norms[0].weight), h16(norms[1].weight)
                self.qk_eps = norms[2]
        self._init_runtime(window=window, kv_cache=kv_cache, inv_freq=inv_freq, att_scale=att_scale, single_copy=False)
        return self

    @staticmethod
    def _hf_qk_norm(attn, head_dim):
        """(q_norm, k_norm, eps) of an attention module that normalises every head of q and k over head_dim in front of the
        rotation (Qwen3), None if it has no such pair.  As for input_layernorm the arithmetic is checked on numbers -- the
        formula of qk_norm.py with the module's own eps, on an input of ordinary size and on one small enough for eps to
        matter -- not on a class name; a weight of any other length (OLMo2 normalises the whole width) is refused."""
        qn, kn = getattr(attn, "q_norm", None), getattr(attn, "k_norm", None)
        if isinstance(qn, torch.nn.Identity) and isinstance(kn, torch.nn.Identity):
            qn = kn = None
        if qn is None and kn is None:
            return None
        if qn is None or kn is None:
            raise NotImplementedError("q_norm without k_norm (or the reverse)")
        eps = None
        for n in (qn, kn):
            w = getattr(n, "weight", None)
            if w is None or w.dim() != 1 or w.numel() != head_dim:
                raise NotImplementedError(f"{type(n).__name__} with a weight of shape "
                                          f"{None if w is None else tuple(w.shape)}: only a norm over head_dim = {head_dim}")
            e = getattr(n, "variance_epsilon", None)
            e = getattr(n, "eps", None) if e is None else e
            if e is None or getattr(n, "bias", None) is not None or (eps is not None and float(e) != eps):
                raise NotImplementedError(f"{type(n).__name__}: no eps attribute, a bias, or two different eps")
            eps = float(e)
            with torch.no_grad():
                for amp in (1.0, 1e-3):
                    xt = amp * torch.linspace(-2.0, 3.0, head_dim, dtype=torch.float32, device=w.device)[None]
                    xt = xt.to(w.dtype).float()
                    want = xt / torch.sqrt((xt * xt).mean() + eps) * w.float()
                    if not torch.allclose(n(xt.to(w.dtype)).float(), want, rtol=2e-2, atol=2e-2):
                        raise NotImplementedError(f"{type(n).__name__} is not RMSNorm(x) * weight over head_dim")
        return qn, kn, eps

    def _init_runtime(self, window=None, kv_cache=None, inv_freq=None, att_scale=1.0, single_copy=False):
        """Everything but the model (s, dev, max_len, embed, lm_head, final_norm, layers: the constructors' part).  Receives
        what differs between the constructors: the attention window, `kv_cache` = (keys, values) to use instead of an own
        cache, the rotary frequencies (None: from rope_theta) with their attention scaling, and single_copy.  EVERY attribute
        the class reads is assigned here.  Called again without arguments -- after max_len was changed: the prompt-pass
        benchmark -- it keeps `window` and `single_copy` as the attributes stand now and the other three as they were given."""
        if window is None:
            window, single_copy = self.window, self.single_copy
            kv_cache, inv_freq, att_scale = self._init_args
        self._init_args = (kv_cache, inv_freq, att_scale)
        s, max_len = self.s, self.max_len
        self.single_copy = bool(single_copy)
        self.window = int(window)            # sliding-window attention: keys (pos - window, pos]; 0 = all
        if kv_cache is not None:
            self.kcache, self.vcache = self._check_kv(*kv_cache)
        else:
            self.kcache = torch.zeros(s.layers, s.kv_heads, max_len, s.head_dim, dtype=torch.float16, device=self.dev)
            self.vcache = torch.zeros_like(self.kcache)
        if inv_freq is None:
            inv_freq = 1.0 / (s.rope_theta ** (torch.arange(0, s.head_dim, 2, dtype=torch.float32) / s.head_dim))
        ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv_freq[None, :]
        self.cos = (torch.cat([ang.cos(), ang.cos()], -1) * float(att_scale)).to(self.dev)     # (max_len, head_dim) fp32
        self.sin = (torch.cat([ang.sin(), ang.sin()], -1) * float(att_scale)).to(self.dev)
        self.arange = torch.arange(max_len, device=self.dev)
        # static step I/O (graph capture): current token id, its position, next token id
        self.tok = torch.zeros(1, dtype=torch.long, device=self.dev)
        self.pos = torch.zeros(1, dtype=torch.long, device=self.dev)
        self.graph = None                   # the captured step and its static logits (capture())
        self.step_logits = None
        self.sampling = None
        self._fed = None                    # host-side count of the tokens generate() fed (generate(append=True))
        self._tail_logits = None            # the whole-token launch's one logits row (step())
        self._prefill_graphs, self._extend_graphs = {}, {}      # length -> (graph, logits, static tokens)
        self._spec = None                   # device state of generate_speculative (_spec_state)
        self._spec_graphs = {}              # (k, gmin, gmax, adapter) -> the captured pass
        self.spec_stats = None              # what the last generate_speculative call did
        self._rm_scratch = {}               # projection name -> row-major scratch (_row_major)
        self.fused_attention = s.head_dim in (64, 128)
        # per-head RMSNorm of q / k in front of the rotation (Qwen3): the layer dicts carry q_norm / k_norm.  qk_fused: the bs = 1
        # and the contiguous batched decode step normalise inside the attention launch (quip_lib::rope_attn_decode_qknorm /
        # _batched_qknorm); off (QUIP_QK_NORM_FUSED=0, or the attribute with `graph = None`): quip_lib::qk_norm_rows in front of
        # the plain launch, the same bits -- the A/B of tools/qk_norm_bench.py.  Every other route takes the launch in front.
        self.qk_norm = "q_norm" in self.layers[0]
        # LoRA adapters (enable_lora): the state lives on through a re-run; with it the persistent launches, the _z attention
        # launch and the token tail stay off, as on a q / k norm model (no adapter branch inside them: not built)
        self.lora = getattr(self, "lora", None)
        # bs = 1 with adapters: the chain / prologue route (_step_fused) where the decoder has one, else _block.  Measured on the
        # 7B shape (tools/lora_bench.py, profiles/lora_bench.txt): _step_fused is 262 us (r 16 on q, v) and 183 us (r 16 on all
        # seven) per token faster than _block, spreads below 5 us.  False (with `graph = None`): _block, for A/B.
        self.lora_fused_step = True
        self._lora_dependents = getattr(self, "_lora_dependents", None) or weakref.WeakSet()    # batched decoders: their captured steps
        self.qk_fused = os.environ.get("QUIP_QK_NORM_FUSED", "1") != "0"
        if self.qk_norm and not self.fused_attention:
            raise NotImplementedError(f"q_norm / k_norm with head_dim {s.head_dim}: the norm launches serve 64 and 128")
        self.attn_ws = _R.rope_attn_workspace(s.heads, s.head_dim, self.dev) if self.fused_attention else None
        L0 = self.layers[0]
        qkv0, gu0 = [L0["q"], L0["k"], L0["v"]], [L0["gate"], L0["up"]]
        planes_ok = all(hasattr(m.codebook, "mm_planes") and m.codebook.planes_supported(m.q_out_features, m.q_in_features)
                        for m in L0.values() if isinstance(m, QuantLinear))
        # stage-wise step (10 launches per block): chain launches where the shapes allow, else the GEMV prologue
        self.chain = (planes_ok and os.environ.get("QUIP_CHAIN", "1") != "0"
                      and chain_supported(qkv0, L0["down"]) and chain_supported(gu0, L0["o"]))
        prologue_ok = (planes_ok and fused_in_supported(qkv0, prev=L0["down"]) and fused_in_supported(gu0, prev=L0["o"]))
        self.o_fused = planes_ok and fused_in_supported([L0["o"]])
        self.qkv_fused = planes_ok and fused_in_supported(qkv0)
        self.fused_prologue = os.environ.get("QUIP_FUSED_PROLOGUE", "1") != "0" and (self.chain or prologue_ok)
        # the MLP half of a block (GEMV[gate, up], two transforms, GEMV[down]) as ONE persistent launch
        # (csrc/decode_engine.hip); QUIP_FFN_ENGINE=0 keeps the four stage-wise launches
        self.ffn_eng = (self.fused_prologue and self.chain and os.environ.get("QUIP_FFN_ENGINE", "1") != "0"
                        and self.lora is None
                        and all(ffn_engine_ok(L["gate"], L["up"], L["down"]) for L in self.layers))
        self.ffn_ws = _R.ffn_engine_workspace(s.ffn, L0["gate"].K_right, self.dev) if self.ffn_eng else None
        # all blocks of a token as ONE persistent launch (csrc/decode_block.hip); QUIP_BLOCK_ENGINE=0 keeps the stage-wise step
        # (E8P12; D4 through the same kernel's one-table mode; E8P12RVQ4B, E8P12RVQ3B and HI as rows of twice the virtual width).
        # What _init_block_engine fills in when every block qualifies:
        self.block_eng = False
        self.eng_layers = self.eng_grid = self.eng_grid2 = self.eng_ws = None
        self.eng_codebook, self.eng_resid_scale, self.eng_shape = 0, 0.0, 0
        self._eng_keep = self._eng_sig = self._kv_ptr_host = None
        self.token_tail = os.environ.get("QUIP_TOKEN_TAIL", "1") != "0"     # the token's tail inside that launch (step())
        # shape 0 with E8P12: the launch streams launch-tiled copies of the codes (QUIP_ENG_TILED=0: the checkpoint's layout, for A/B);
        # read once, so that a rebuild of the descriptors (reset()) keeps the layout the decoder was built with
        self.eng_tiled = os.environ.get("QUIP_ENG_TILED", "1") != "0"
        d4 = all(getattr(m.codebook, "id", None) in ("D4", "E8P12RVQ4B", "HI", "E8P12RVQ3B") for m in L0.values() if isinstance(m, QuantLinear))
        gqa_shape = self.fused_prologue and self.chain and s.kv_heads != s.heads and s.hidden in (8192, 4096)   # (csrc/decode_block_gqa.hip; decode_block_g8.hip)
        if ((self.ffn_eng or gqa_shape or (d4 and self.fused_prologue and self.chain and os.environ.get("QUIP_FFN_ENGINE", "1") != "0"))
                and os.environ.get("QUIP_BLOCK_ENGINE", "1") != "0" and not self.window     # (its attention walks [0, pos])
                and not self.qk_norm                # (the persistent launches have no q / k norm: not built)
                and self.lora is None):             # (nor an adapter branch)
            self._init_block_engine()
        # q / k / v output transforms inside the attention launch (multi-head attention with a power-of-two hidden <= 4096,
        # or 64 / 32 heads on 8 KV heads -- Llama-2-70B, Llama-3, Mistral-7B; plain SV output side)
        self.attn_z = (self.fused_prologue and self.fused_attention and os.environ.get("QUIP_ATTN_Z", "1") != "0"
                       and not self.qk_norm                 # (the _z launch has no q / k norm: not built)
                       and self.lora is None                # (adapters add to the materialised q / k / v)
                       and _R.rope_attn_decode_z_supported(s.heads, s.kv_heads, s.head_dim)
                       and all(l.K_right == 1 and not l.per_channel and l.bias is None and l.SV is not None
                               and l.q_out_features == l.out_features == (s.heads if i == 0 else s.kv_heads) * s.head_dim
                               for i, l in enumerate(qkv0)))

    def _init_block_engine(self):
        """descriptors + workspace of the persistent block launch, when every block qualifies"""
        s, L0 = self.s, self.layers[0]
        cbid = getattr(L0["q"].codebook, "id", None)
        if cbid not in _ENGINE_CODEBOOK:
            return

        def plain(m, n_in, n_out):
            return (getattr(m.codebook, "id", None) == cbid and not m.per_channel and m.bias is None and not m.training
                    and m.SU is not None and m.SV is not None and m.in_features == m.q_in_features == n_in
                    and m.out_features == m.q_out_features == n_out)
        with torch.cuda.device(self.dev):           # (the support queries ask the CURRENT device for its CU count)
            dims = (s.hidden, s.heads, s.kv_heads, s.head_dim, s.ffn, L0["gate"].K_right)
            gqa = _R.block_engine_gqa_supported(*dims) and cbid == "E8P12"        # shape 1: the 8192-wide launch
            # shape 2: Llama-3-8B / Mistral-7B -- the shape-0 launch compiled for 32 / 8 heads and n_ffn = 14336 = 56 x 256
            g8 = (not gqa and cbid == "E8P12" and os.environ.get("QUIP_BLOCK_ENGINE_G8", "1") != "0" and not self.window
                  and _R.block_engine_g8_supported(*dims))
            ok = ((gqa or g8 or _R.block_engine_supported(*dims)) and s.q_width == s.hidden and not self.qk_norm
                  and len(self.layers) <= 146)      # (the launch's hand-off counter: 7 per block in 10 bits)
            kvw = s.kv_heads * s.head_dim
            for L in self.layers:
                ok = ok and all(plain(L[k], s.hidden, s.hidden) and L[k].K_left == 1 and L[k].K_right == 1 for k in "qo")
                ok = ok and all(plain(L[k], s.hidden, kvw) and L[k].K_left == 1 and L[k].K_right == 1 for k in "kv")
                ok = ok and all(plain(L[k], s.hidden, s.ffn) and L[k].K_left == 1 for k in ("gate", "up"))
                ok = ok and plain(L["down"], s.ffn, s.hidden) and L["down"].K_right == 1
            if not ok:
                return
            # shape 0 with E8P12 streams launch-tiled copies of the codes (codebook id 5; QUIP_ENG_TILED=0: the checkpoint's layout,
            # id 0, for A/B).  They live in _eng_keep only: `Qidxs` stays the truth (_engine_signature reads ITS pointer and version)
            launch_tiled = not gqa and not g8 and cbid == "E8P12" and self.eng_tiled
            keep, rec = [], np.zeros((len(self.layers), 32), dtype=np.uint64)
            # (a rebuild -- reset() after the modules were edited: the previous descriptors' tensors, for shape 1 a whole tiled
            #  copy of the codes, go BEFORE the new ones are made, not after: no third copy of the weights in between)
            self._eng_keep = None
            self.eng_layers = None
            for i, L in enumerate(self.layers):
                mods = [L[k] for k in PROJECTIONS]
                su, sv, ln = _engine_vectors(L, 16 if gqa else 8)
                had3 = _had3_mix(L, self.dev) if gqa else (_had3_k56(L, self.dev) if g8
                                                           else _engine_had3(L["gate"], L["up"], L["down"]))
                wq = (_tiled_codes(mods, self.single_copy) if gqa else
                      (_launch_tiled_codes(L) if launch_tiled else [m.Qidxs for m in mods]))
                keep += su + sv + ln + [had3] + (wq if gqa or launch_tiled else [])
                ptrs = ([t.data_ptr() for t in wq] + [t.data_ptr() for t in ln] + [t.data_ptr() for t in su]
                        + [t.data_ptr() for t in sv] + [had3.data_ptr(), self.kcache[i].data_ptr(), self.vcache[i].data_ptr()])
                rec[i, :26] = np.array(ptrs, dtype=np.uint64)
                sc = [m.wscale_float / math.sqrt(m.q_in_features // m.K_left) for m in mods]
                rec[i, 26:].view(np.float32)[:7] = np.array(sc, dtype=np.float32)
            self._eng_keep = keep
            self.eng_layers = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).to(self.dev)
            self.eng_shape = 1 if gqa else (2 if g8 else 0)
            self.eng_ws = _R.block_engine_workspace(self.dev, self.eng_shape)
            self.eng_codebook = _ENGINE_CODEBOOK_TILED if launch_tiled else _ENGINE_CODEBOOK[cbid]
            cb0 = L0["q"].codebook
            self.eng_grid = cb0.grid if cbid == "D4" else (cb0._virtual_grid(self.dev) if cbid == "HI" else cb0.grid_packed_abs)
            self.eng_resid_scale = float(getattr(cb0, "planes_resid_scale", 0.0)) if cbid in ("E8P12RVQ4B", "E8P12RVQ3B") else 0.0
            self.eng_grid2 = cb0._e81b_i8(self.dev) if cbid == "E8P12RVQ3B" else None      # int8 (256, 8): 4 x the E81B entries
            self._eng_sig = self._engine_signature()
            self._kv_ptr_host = torch.empty(len(self.layers), 2, dtype=torch.int64).pin_memory()      # (bind_kv's staging buffer)
            self.block_eng = True

    def _engine_signature(self):
        """(data_ptr, version) of every tensor the engine descriptors were built from: a load_state_dict / .to() / in-place
        edit of a module after the descriptors were baked shows up here (reset() rebuilds them then).  Of the codes it is the
        tiled copy where a module has one: its `Qidxs` is None then, or scratch on loan (_row_major)"""
        sig = []
        for L in self.layers:
            for k in PROJECTIONS:
                m = L[k]
                tiled = getattr(m, "_qidxs_tiled", None)
                for t in (tiled if tiled is not None else m.Qidxs, m.SU, m.SV, m.had_left, m.had_right):
                    if t is not None:
                        sig.append((t.data_ptr(), t._version))
                sig.append(float(m.wscale_float))
            sig += [(L["ln1"].data_ptr(), L["ln1"]._version), (L["ln2"].data_ptr(), L["ln2"]._version)]
        return tuple(sig)

    def engine_status(self):
        """0, or the code of a wait that gave up inside a persistent launch (synchronises)"""
        for ws in (self.eng_ws, self.ffn_ws):
            if ws is not None and _R.ffn_engine_status(ws) != 0:
                return _R.ffn_engine_status(ws)
        return 0

    def engine_fail_position(self):
        """position of the first token a persistent block launch did not compute (workspace word 2 - 1), or None"""
        if self.eng_ws is None:
            return None
        v = int(self.eng_ws[8:12].view(torch.int32).item())
        return v - 1 if v > 0 else None

    def _check_kv(self, keys, values):
        s = self.s
        keys, values = list(keys), list(values)
        if len(keys) != s.layers or len(values) != s.layers:
            raise ValueError(f"kv_cache: {s.layers} key and value tensors expected")
        for t in keys + values:
            if (tuple(t.shape) != (s.kv_heads, self.max_len, s.head_dim) or t.dtype != torch.float16 or not t.is_contiguous()
                    or t.device != self.dev):
                raise ValueError(f"kv_cache tensors: contiguous fp16 ({s.kv_heads}, {self.max_len}, {s.head_dim}) on {self.dev}")
        return keys, values

    def bind_kv(self, keys, values):
        """use other cache tensors (same shapes) from now on: the stage-wise step reads self.kcache[i] at every call; the
        block launch's descriptors hold the row pointers (words 24, 25 of a 256-byte descriptor) and are patched in place;
        a captured step is dropped (its launches hold the old pointers)"""
        self.kcache, self.vcache = self._check_kv(keys, values)
        if self.block_eng:
            # through a pinned staging buffer that lives as long as the decoder: the copy is legal inside a stream capture
            # (a re-recording torch.compile graph meets a new cache object there) and replays read the same host memory
            host = self._kv_ptr_host
            for i, (k, v) in enumerate(zip(self.kcache, self.vcache)):
                host[i, 0], host[i, 1] = k.data_ptr(), v.data_ptr()
            rec = self.eng_layers.view(torch.int64).view(len(self.layers), 32)
            rec[:, 24:26].copy_(host, non_blocking=True)
        self.graph = None

    def engine_reset(self):
        """after a launch that gave up: workspaces back to their allocation state (generation 0, no granules, no code)"""
        for ws in (self.eng_ws, self.ffn_ws):
            if ws is not None:
                ws.zero_()

    def _engine_recover(self):
        """The one answer to a persistent launch that gave up.  Such a launch -- its workgroups were not all resident: something
        else on the device -- ends on a hand-off instead of hanging, leaves a code in its workspace, answers NaN and remembers
        the position of the first token it did not compute.  Reads the status (synchronises), zeroes the workspaces and, unless
        the code only says that the workspace wanted zeroing (its launch counter was about to wrap), warns, switches both
        persistent launches off and drops the captured step.  Returns (code, that position or None); code 0: nothing
        happened, anything else: the caller repeats what it ran, on the path this decoder is on now."""
        if not (self.block_eng or self.ffn_eng):
            return 0, None
        st = self.engine_status()
        if not st:
            return 0, None
        fail = self.engine_fail_position()
        self.engine_reset()
        if st != 0xE000:
            warnings.warn("persistent decode launch gave up on a hand-off (code 0x%x): the device was shared with other "
                          "work; decoding continues on the stage-wise step" % st)
            self.block_eng = self.ffn_eng = False
            self.graph = None
        return st, fail

    # ---- single-copy mode: a block's matrices in the checkpoint's layout, for the operators that read it ------------------------
    @contextmanager
    def _row_major(self, L):
        """inside the `with`, the seven modules of block L have their row-major `Qidxs` back (in scratch buffers shared by all
        blocks, filled by untile_codes on the current stream); handed back on the way out, whatever happens inside.  Does
        nothing unless the modules hold tiled copies only."""
        if not self.single_copy:
            yield
            return
        lent = []
        try:
            for k in PROJECTIONS:
                m = L[k]
                if m.Qidxs is None and getattr(m, "_qidxs_tiled", None) is not None:
                    shape, dtype = m._qidxs_meta
                    buf = self._rm_scratch.get(k)
                    if buf is None or tuple(buf.shape) != shape or buf.dtype != dtype:
                        buf = self._rm_scratch[k] = torch.empty(shape, dtype=dtype, device=self.dev)
                    untile_codes(m._qidxs_tiled, shape[0], buf.numel() * buf.element_size() // shape[0], buf)
                    m.Qidxs = buf
                    lent.append(m)
            yield
        finally:
            for m in lent:
                m.Qidxs = None

    # ---- model bytes the decode step has to stream (roofline denominator) -----------
    def algorithmic_bytes_per_token(self):
        b = 0
        for L in self.layers:
            for k in PROJECTIONS:
                m = L[k]
                b += qidxs_nbytes(m) + 2 * (m.in_features + m.out_features)
        return b + self.lm_head.numel() * 2

    def _rope(self, x, cos, sin):
        d = x.shape[-1] // 2
        rot = torch.cat([-x[..., d:], x[..., :d]], -1)
        return (x.float() * cos + rot.float() * sin).to(x.dtype)

    def _attention(self, i, q, k, v, cos, sin, mask):
        s = self.s
        if self.qk_norm and self.qk_fused:
            # the same launch with q and the new k row normalised in registers in front of the rotation
            L = self.layers[i]
            return torch.ops.quip_lib.rope_attn_decode_qknorm(
                q.view(s.heads, s.head_dim), k.view(s.kv_heads, s.head_dim), v.view(s.kv_heads, s.head_dim),
                self.cos, self.sin, self.pos, self.kcache[i], self.vcache[i], self.attn_ws, self.window,
                L["q_norm"], L["k_norm"], self.qk_eps)
        if self.qk_norm:
            q, k = self._qk_norm_rows(self.layers[i], q, k)
        if self.fused_attention:
            # rope + cache append + attention over [0, pos]: one launch
            return torch.ops.quip_lib.rope_attn_decode(
                q.view(s.heads, s.head_dim), k.view(s.kv_heads, s.head_dim), v.view(s.kv_heads, s.head_dim),
                self.cos, self.sin, self.pos, self.kcache[i], self.vcache[i], self.attn_ws, self.window)
        q = self._rope(q.view(1, s.heads, 1, s.head_dim), cos, sin)
        k = self._rope(k.view(1, s.kv_heads, 1, s.head_dim), cos, sin)
        self.kcache[i].index_copy_(1, self.pos, k[0])
        self.vcache[i].index_copy_(1, self.pos, v.view(s.kv_heads, 1, s.head_dim))
        return F.scaled_dot_product_attention(q, self.kcache[i][None], self.vcache[i][None], attn_mask=mask,
                                              enable_gqa=(s.kv_heads != s.heads))

    def _qk_norm_rows(self, L, q, k):
        """q (rows, heads * hd) and k (rows, kv_heads * hd) with every head normalised (quip_lib::qk_norm_rows: in place, one
        launch for both)"""
        s = self.s
        q, k = q.reshape(-1, s.q_width).contiguous(), k.reshape(-1, s.kv_heads * s.head_dim).contiguous()
        torch.ops.quip_lib.qk_norm_rows(q, k, L["q_norm"], L["k_norm"], s.head_dim, self.qk_eps)
        return q, k

    def _block(self, L, h, attend, norm_in_attend=False, adapter=None):
        """one decoder block on the rows of `h`, stage by stage; `attend(q, k, v)` -> the attention output, (rows, heads *
        head_dim): the decode step, the prompt passes and BatchDecoder.step differ in nothing else.  A model with q / k norms
        gets them here, behind the projections (quip_lib::qk_norm_rows), unless `norm_in_attend`: that `attend` takes the raw
        q and k and normalises them itself (the decode launches that fuse the norm).
        `adapter` (enable_lora): the int32 adapter index of every row of `h`, on the device.  q / k / v and gate / up: one
        shrink over the group's stacked ranks with the norm fused, the base product, one expand over the group's outputs.
        o and down: their input shrunk (down's with the gate) and the delta expanded INTO THE RESIDUAL (h, in place) in
        front of the module's output launch, which adds the residual as ever -- the same sum, and nothing has to follow
        the output-side launch.  A group no loaded adapter targets launches nothing."""
        s = self.s
        lo = L["lora"] if adapter is not None and self.lora is not None else None
        with self._row_major(L):
            # q / k / v (and gate / up below): one launch per stage for the whole group; RMSNorm rides on
            # the input-side Hadamard launch
            t = lo.shrink("qkv", h, adapter, rms_weight=L["ln1"], rms_eps=s.rms_eps) if lo else None
            q, k, v = forward_group([L["q"], L["k"], L["v"]], h, rms_weight=L["ln1"], rms_eps=s.rms_eps)
            if t is not None:
                lo.expand("qkv", t, [q, k, v], adapter)
            if self.qk_norm and not norm_in_attend:
                q, k = self._qk_norm_rows(L, q, k)
            # residual adds ride on the output-side Hadamard launch, SiLU(gate)*up on down's input side
            a = attend(q, k, v)
            t = lo.shrink("o", a, adapter) if lo else None
            if t is not None:
                lo.expand("o", t, [h], adapter)
            h = L["o"].forward_fused(a, residual=h)
            t = lo.shrink("gu", h, adapter, rms_weight=L["ln2"], rms_eps=s.rms_eps) if lo else None
            g, u = forward_group([L["gate"], L["up"]], h, rms_weight=L["ln2"], rms_eps=s.rms_eps)
            if t is not None:
                lo.expand("gu", t, [g, u], adapter)
            t = lo.shrink("down", u, adapter, gate=g) if lo else None
            if t is not None:
                lo.expand("down", t, [h], adapter)
            return L["down"].forward_fused(u, gate=g, residual=h)

    # ---- LoRA adapters (lora.py) ---------------------------------------------------------------------------------------------
    def enable_lora(self, max_adapters=4, max_rank=16):
        """Adapter slots beside every QuantLinear of every block: the stacked A / B / scale tensors of `max_adapters`
        adapters of rank <= `max_rank` (padded to a multiple of 8), allocated once, zero-filled, at fixed addresses -- a
        captured step survives load_adapter / unload_adapter / set_adapter.  From here on the persistent launches, the
        _z attention launch and the token tail are off and the captured steps are dropped.  Without this call nothing
        changes; with it and no adapter selected, every result keeps its bits."""
        if self.lora is not None:
            raise RuntimeError("enable_lora: already enabled")
        lora = _lora.LoraState(self, max_adapters, max_rank)
        for L, lay in zip(self.layers, lora.layers):
            L["lora"] = lay
        lora.on_launches_changed = self._drop_graphs
        self.lora = lora
        self.block_eng = self.ffn_eng = self.attn_z = False
        self.eng_layers = self._eng_keep = None
        self._drop_graphs()

    def _drop_graphs(self):
        """captured steps and passes hold launch lists: gone when the groups that launch change"""
        self.graph = None
        self._prefill_graphs, self._extend_graphs, self._spec_graphs = {}, {}, {}
        for d in list(self._lora_dependents):
            d.graph = None

    def _need_lora(self):
        if self.lora is None:
            raise RuntimeError("no adapter slots: call enable_lora() first")
        return self.lora

    def load_adapter(self, name, tensors, config):
        """an adapter in PEFT's key scheme (lora.read_peft_dir; lora.check_config says what is served) into a slot -> the
        slot's index.  A loaded name is replaced in its slot.  Captured steps are kept unless the adapter targets a module
        group no loaded adapter targeted before (that group's launches join the step)."""
        return self._need_lora().load(name, tensors, config)

    def unload_adapter(self, name):
        """zero the adapter's stack entry and free its slot"""
        self._need_lora().unload(name)

    def set_adapter(self, name):
        """the bs = 1 decoder's adapter from now on (None: none): an int32 on the device that step(), captured or not, and
        the prompt passes read in place"""
        self._need_lora().idx.fill_(self.lora.index(name))

    def _rows_adapter(self, adapter, n):
        """the per-row adapter index _block wants for n rows of one sequence, from its (1,) index tensor (default: the
        bs = 1 decoder's); None without enable_lora.  Nothing is read on the host."""
        if self.lora is None:
            return None
        adapter = self.lora.idx if adapter is None else adapter
        return adapter if n == 1 else adapter.expand(n).contiguous()

    def _engine_args(self):
        """the arguments quip_lib::block_engine and quip_lib::block_engine_token share: everything behind their own I/O"""
        s = self.s
        return (self.cos, self.sin, self.eng_grid, self.eng_ws, len(self.layers), self.max_len, s.rms_eps,
                1.0 / math.sqrt(s.head_dim), None, -1, self.eng_codebook, self.eng_resid_scale, self.eng_shape, self.eng_grid2,
                *((self.kcache, self.vcache) if torch.is_tensor(self.kcache) else (None, None)))

    def step(self):
        """one token: reads self.tok / self.pos, writes the greedy next token into self.tok and
        advances self.pos (all on the device)"""
        s = self.s
        if self._token_tail_on():
            # the whole token in ONE launch: embedding row, blocks, final norm, lm_head, arg-max, position (csrc/token_tail.hip.h)
            lg = self._tail_logits
            if lg is None or lg.shape[1] != self.lm_head.shape[0] or lg.device != self.lm_head.device:
                lg = self._tail_logits = torch.empty(1, self.lm_head.shape[0], dtype=torch.float16, device=self.lm_head.device)
            torch.ops.quip_lib.block_engine_token(self.eng_layers, self.tok, self.pos, self.embed, self.final_norm, self.lm_head,
                                                  lg, *self._engine_args())
            return lg
        h = self.embed[self.tok]                                   # (1, hidden)
        cos = sin = mask = None
        if not self.fused_attention:
            cos, sin = self.cos[self.pos], self.sin[self.pos]          # (1, head_dim)
            mask = (self.arange[None, None, None, :] <= self.pos)      # (1,1,1,max_len) keys <= current
            if self.window:
                mask = mask & (self.arange[None, None, None, :] > self.pos - self.window)
        if self.block_eng:
            h = torch.ops.quip_lib.block_engine(self.eng_layers, h.reshape(-1), self.pos, *self._engine_args())
            return self._head(h.reshape(1, -1))
        if self.fused_prologue and (self.lora is None or self.lora_fused_step):
            return self._step_fused(h, cos, sin, mask)

        def attend(i, q, k, v):
            return self._attention(i, q, k, v, cos, sin, mask).reshape(1, s.q_width)
        for i, L in enumerate(self.layers):
            h = self._block(L, h, partial(attend, i), norm_in_attend=True,     # (_attention: fused, or the launch in front)
                            adapter=self._rows_adapter(None, 1))
        return self._head(h)

    def _token_tail_on(self):
        """greedy decoding on the 4096-wide persistent launch: the tail of the token rides on it.  QUIP_TOKEN_TAIL=0 (read
        when the runtime state is built; `token_tail` afterwards, with `graph = None`) keeps the separate launches."""
        if not (self.block_eng and self.token_tail and self.sampling is None and self.eng_shape in (0, 2)):
            return False
        lm, em = self.lm_head, self.embed
        return (lm.is_cuda and lm.dtype == torch.float16 and lm.is_contiguous() and lm.dim() == 2 and lm.shape[1] == 4096
                and 256 <= lm.shape[0] < 256 * 65535 and em.dtype == torch.float16 and em.is_contiguous()
                and em.shape == lm.shape and em.device == lm.device and self.final_norm.dtype == torch.float16
                and self.final_norm.is_contiguous() and len(self.layers) <= 146)

    def _step_fused(self, h, cos, sin, mask):
        """8 launches per block: the GEMV launches of q/k/v, o and gate/up compute their own input
        transform (RMSNorm, SU, Hadamard) and the output transform + residual of the module before
        them (down of the previous block, o) in their prologue.
        With adapters (enable_lora and lora_fused_step; ffn_eng and attn_z are off then) the hooks of _block: the shrink on
        the h a launch returns or takes, the expand on the materialised q / k / v and gate / up, o's and down's delta into
        the residual h (in place) in front of the launch that adds it."""
        s = self.s
        zd = prev_down = None
        ad = self.lora.idx if self.lora is not None else None
        for i, L in enumerate(self.layers):
            lo = L["lora"] if ad is not None else None
            with self._row_major(L):
                qkv = [L["q"], L["k"], L["v"]]
                if zd is None and self.qkv_fused:
                    _, zs = gemv_fused(qkv, x=h, rms_weight=L["ln1"], rms_eps=s.rms_eps)
                elif zd is None:
                    zs = gemv_group_unfused(qkv, h, rms_weight=L["ln1"], rms_eps=s.rms_eps)
                else:   # finishes the previous block: h += down(...)
                    h, zs = self._zx(qkv, prev_down, zd, h, L["ln1"])
                t = lo.shrink("qkv", h, ad, rms_weight=L["ln1"], rms_eps=s.rms_eps) if lo else None
                if self.attn_z:
                    # the K = 1 output transforms of q / k / v in the attention launch's prologue: 9 launches per block
                    a = torch.ops.quip_lib.rope_attn_decode_z(
                        list(zs), [l._vec(l.SV) for l in qkv], [1.0 / math.sqrt(l.q_out_features) for l in qkv],
                        self.cos, self.sin, self.pos, self.kcache[i], self.vcache[i], self.attn_ws, self.window)
                else:
                    q, k, v = out_transform_group(qkv, zs)
                    if t is not None:
                        lo.expand("qkv", t, [q, k, v], ad)
                    a = self._attention(i, q, k, v, cos, sin, mask)
                t = lo.shrink("o", a.reshape(1, s.q_width), ad) if lo else None
                if t is not None:
                    lo.expand("o", t, [h], ad)
                if self.o_fused:
                    _, (zo,) = gemv_fused([L["o"]], x=a.reshape(1, s.q_width))
                else:
                    zo = gemv_unfused(L["o"], a.reshape(1, s.q_width))
                if self.ffn_eng:
                    h, planes = chain_planes([L["gate"], L["up"]], L["o"], zo, residual=h, rms_weight=L["ln2"],
                                             rms_eps=s.rms_eps)
                    zd = ffn_engine(L["gate"], L["up"], L["down"], planes, self.ffn_ws)
                else:
                    h, zgu = self._zx([L["gate"], L["up"]], L["o"], zo, h, L["ln2"])
                    t = lo.shrink("gu", h, ad, rms_weight=L["ln2"], rms_eps=s.rms_eps) if lo else None
                    g, u = out_transform_group([L["gate"], L["up"]], zgu)
                    if t is not None:
                        lo.expand("gu", t, [g, u], ad)
                    t = lo.shrink("down", u, ad, gate=g) if lo else None
                    if t is not None:
                        lo.expand("down", t, [h], ad)
                    zd = gemv_unfused(L["down"], u, gate=g)
                prev_down = L["down"]
        (h,) = out_transform_group([prev_down], [zd], residual=[h])
        return self._head(h)

    def _zx(self, layers, prev, z, residual, ln):
        """producer's output side + consumers' input side + GEMV: as a Hadamard chain launch (one
        workgroup per consumer, in parallel) followed by the grouped GEMV, or inside the GEMV
        prologue (every workgroup repeats all transforms one after the other)"""
        if self.chain:
            return gemv_chain(layers, prev, z, residual=residual, rms_weight=ln, rms_eps=self.s.rms_eps)
        return gemv_fused(layers, prev=prev, z=z, residual=residual, rms_weight=ln, rms_eps=self.s.rms_eps)

    def set_sampling(self, temperature=None, top_k=None):
        """greedy (default, temperature None / 0) or the reference demo's sampler
        (example_generate.py:9-26: logits / T, optional top-k cut, softmax, exponential-race arg-max --
        no host synchronisation).  The choice is part of the captured step: changing it re-captures."""
        new = None if not temperature else (float(temperature), None if top_k is None else int(top_k))
        if new != self.sampling:
            self.sampling, self.graph = new, None

    def _head(self, h):
        s = self.s
        logits = F.rms_norm(h, (s.hidden,), self.final_norm, s.rms_eps) @ self.lm_head.T
        if self.sampling is None:
            if logits.dtype == torch.float16 and logits.is_cuda:
                torch.ops.quip_lib.argmax_step(logits, self.tok, self.pos)      # tok <- argmax, pos += 1: one launch
                return logits
            self.tok.copy_(logits.argmax(-1))
        else:
            self.tok.copy_(self.sample(logits, *self.sampling))
        self.pos.add_(1)
        return logits

    @staticmethod
    def sample(logits, temperature, top_k):
        """one token per row of `logits` (rows, vocab): the sampler of set_sampling"""
        lg = logits.float() / max(temperature, 1e-5)
        if top_k is not None:
            v, _ = torch.topk(lg, min(top_k, lg.size(-1)))
            lg = torch.where(lg < v[..., -1:], -float("inf"), lg)
        probs = torch.softmax(lg, dim=-1)
        q = torch.empty_like(probs).exponential_(1)
        return torch.argmax(probs / q, dim=-1)

    def batched(self, batch, max_len=None, paged=False, pages=None, kv_dtype=None, kv_exp=None, padded=False):
        """a decoder of `batch` independent sequences on this decoder's modules (batch_decode.BatchDecoder); paged: its
        KV cache is a pool of `pages` 64-position pages shared by the slots (paged_cache.PagedBatchDecoder; default: as
        many pages as the contiguous cache has rows for).  kv_dtype="fp8" (paged only): the pools hold one OCP e4m3fn
        byte per element, kv_exp the (layers, 2) power-of-two exponents of K | V (default 0; see paged_cache).
        padded (contiguous cache only): every slot has a first cache row `start[b]` of its own -- the layout of a
        left-padded HF generate batch; step / decode / capture / reset only (see BatchDecoder)"""
        if paged and padded:
            raise ValueError("padded=True: only with the contiguous cache (paged=False)")
        if paged:
            from .paged_cache import PagedBatchDecoder
            return PagedBatchDecoder(self, batch, max_len, pages, kv_dtype, kv_exp)
        if kv_dtype not in (None, "fp16") or kv_exp is not None:
            raise ValueError("kv_dtype='fp8' / kv_exp: only with paged=True")
        if pages is not None:
            raise ValueError("pages: only with paged=True")
        from .batch_decode import BatchDecoder
        return BatchDecoder(self, batch, max_len, padded=bool(padded))

    prefill_graph_cache_size = 8      # captured prompt lengths kept (each graph owns a memory pool)

    def _replay_per_length(self, cache, tokens, warmup, run):
        """run(tokens) replayed from the graph `cache` holds for this token count; a count met for the first time is captured
        (after warmup(tokens); both get a static copy of the tokens), the oldest one leaving at prefill_graph_cache_size"""
        P = tokens.numel()
        if P not in cache:
            if len(cache) >= self.prefill_graph_cache_size:
                cache.pop(next(iter(cache)))              # oldest captured length out (a graph keeps its own memory pool)
            static_tok = tokens.clone()
            cache[P] = (*capture_graph(lambda: warmup(static_tok), lambda: run(static_tok)), static_tok)
        g, logits, static_tok = cache[P]
        static_tok.copy_(tokens)
        g.replay()
        return logits

    @torch.no_grad()
    def prefill_graph(self, tokens):
        """prefill() replayed from a hipGraph captured per prompt LENGTH (first call of a length captures: a serving
        loop would bucket its prompt lengths).  Short prompts are bound by the ~600 eager launches of the pass, not by
        the GPU: 33..256 tokens 18.7 -> 4..8 ms on the 32-layer 7B model (tools/ttft_bench.py --graph)."""
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        return self._replay_per_length(self._prefill_graphs, tokens, self.prefill, self.prefill)

    def prefill(self, tokens, kv=None, pos=None, adapter=None):
        """Batched prompt pass (the reference demo's prefill, example_generate.py:36-47): all `tokens` (1-D ids) go
        through every block at once -- QuantLinear on (P, hidden) rows (M >= 32: skinny chunks or decompress + dense GEMM, fewer
        rows: the skinny paths), rotary embedding for positions 0..P-1, causal attention, K / V written to rows 0..P-1
        of the static cache -- and the position counter is left at P.  Returns the logits of the last token (1, vocab).
        `kv` = (keys, values): per-layer (kv_heads, >= P, head_dim) tensors to write instead of this decoder's cache, and
        `pos`: the counter to leave at P instead of self.pos (BatchDecoder.prefill_slot: one slot of a batched cache);
        `adapter`: that slot's (1,) adapter index (enable_lora; default: set_adapter's)."""
        s = self.s
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        P = tokens.numel()
        assert 1 <= P <= self.max_len
        kcache, vcache = (self.kcache, self.vcache) if kv is None else kv
        h = self.embed[tokens]                                          # (P, hidden)
        cos, sin = self.cos[:P], self.sin[:P]                           # (P, head_dim)

        def attend(i, q, k, v):
            q = self._rope(q.view(P, s.heads, s.head_dim).transpose(0, 1), cos, sin)          # (heads, P, hd)
            k = self._rope(k.view(P, s.kv_heads, s.head_dim).transpose(0, 1), cos, sin)
            v = v.view(P, s.kv_heads, s.head_dim).transpose(0, 1)
            kcache[i][:, :P].copy_(k)
            vcache[i][:, :P].copy_(v)
            if self.window and P > self.window:     # causal band: key t for query p iff p - window < t <= p
                band = (self.arange[:P, None] >= self.arange[None, :P]) & (self.arange[:P, None] - self.arange[None, :P] < self.window)
                a = F.scaled_dot_product_attention(q[None], k[None], v[None], attn_mask=band,
                                                   enable_gqa=(s.kv_heads != s.heads))[0]
            else:
                a = F.scaled_dot_product_attention(q[None], k[None], v[None], is_causal=True,
                                                   enable_gqa=(s.kv_heads != s.heads))[0]     # (heads, P, hd)
            return a.transpose(0, 1).reshape(P, s.q_width)
        rows_adapter = self._rows_adapter(adapter, P)
        for i, L in enumerate(self.layers):
            h = self._block(L, h, partial(attend, i), adapter=rows_adapter)
        (self.pos if pos is None else pos).fill_(P)
        return F.rms_norm(h[-1:], (s.hidden,), self.final_norm, s.rms_eps) @ self.lm_head.T

    @torch.no_grad()
    def extend(self, tokens, chunk=512, kv=None, pos=None, adapter=None):
        """Append `tokens` (1-D ids, >= 1) behind the current position: the prompt pass for a cache that already holds a
        conversation (a second turn, a prompt too long for one pass, a slot of a batched cache).  The tokens run in chunks
        of at most `chunk` rows -- bounded activations whatever the prompt length -- and per block and chunk the
        attention is ONE launch (quip_lib::rope_attn_chunk: rotary embedding, cache append, causal attention of the
        chunk's rows at positions [pos, pos + rows) over cache rows [0, pos + rows), sliding window included).  The
        position is read by that launch and advanced on the device by each chunk's length: nothing here reads it on the
        host, so the pass can be captured once and replayed at any position (extend_graph).  Tokens that do not fit
        (position + rows > max_len) write nothing and give NaN logits -- the launch's range rule is the guard.
        Returns the logits of the last token (1, vocab).  `kv` / `pos` / `adapter`: as in prefill()."""
        last = [None]

        def keep(c0, h):
            last[0] = h
        _extend_chunks(self, "extend", tokens, chunk, kv, pos, keep, adapter)
        return F.rms_norm(last[0][-1:], (self.s.hidden,), self.final_norm, self.s.rms_eps) @ self.lm_head.T

    @torch.no_grad()
    def score(self, tokens, targets=None, chunk=512, kv=None, pos=None, adapter=None):
        """extend() that scores its tokens: `tokens` go behind the current position exactly as extend() sends them (same
        chunks, same launches, same cache rows and counter, `kv` / `pos` as there -- a cached context conditions the
        scores), and after each chunk ALL its rows take the final norm, the lm_head product and the scoring tail
        (quip_lib::nll_rows: no fp32 copy of the (chunk, vocab) logits).  Row i is scored against targets[i]; the
        default is tokens[1:] followed by -1 -- a negative target means "not scored" and gives exactly 0.  Returns
        (logprob, argmax), both (P,) on the device: log p(targets[i] | context, tokens[:i + 1]) in fp32 and the most
        likely next token of every row.  Nothing is read on the host.  Tokens that do not fit max_len behave as in
        extend(): their rows' logits are NaN, so scored rows give NaN.  QUIP_NLL_ROWS=0 swaps the tail for the torch
        expression (score.nll_rows_torch), for A/B runs."""
        s = self.s
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        if tokens.numel() < 1:
            raise ValueError("score: an empty token list")
        targets = _score.shifted_targets(tokens) if targets is None else \
            torch.as_tensor(targets, dtype=torch.long, device=self.dev).reshape(-1)
        if targets.numel() != tokens.numel():
            raise ValueError(f"score: {targets.numel()} targets for {tokens.numel()} tokens")
        lps, ams = [], []

        def tail(c0, h):
            logits = F.rms_norm(h, (s.hidden,), self.final_norm, s.rms_eps) @ self.lm_head.T
            lp, am = _score.score_tail(logits, targets[c0:c0 + h.shape[0]])
            lps.append(lp)
            ams.append(am)
        _extend_chunks(self, "score", tokens, chunk, kv, pos, tail, adapter)
        return torch.cat(lps), torch.cat(ams)

    @torch.no_grad()
    def perplexity(self, tokens, window=2048, stride=None, chunk=512):
        """Perplexity of `tokens` (1-D ids, >= 2) by the usual protocol (score.plan_score_windows): windows of at most
        `window` tokens start every `stride` tokens (default: window, no overlap), each is scored from position 0 with
        score(), and from the second window on only the rows no earlier window scored count -- the others are context.
        The log-probabilities are summed in float64 on the device; the host reads the totals once, at the end.
        -> {"nll_sum": -sum of log p, "n_scored": counted targets (len(tokens) - 1), "ppl": exp(nll_sum / n_scored),
        "argmax_hits": counted rows whose most likely token is the target}.
        Restores nothing: the cache and the position counter are left at the end of the last window."""
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        plan = _score.plan_score_windows(tokens.numel(), window, stride, max_len=self.max_len)
        total = torch.zeros((), dtype=torch.float64, device=self.dev)
        hits = torch.zeros((), dtype=torch.long, device=self.dev)
        n_scored = 0
        for start, length, first in plan:
            targets = tokens[start + 1:start + length + 1].clone()
            targets[:first] = -1                                        # context rows: exactly 0, never a hit
            self.pos.zero_()
            lp, am = self.score(tokens[start:start + length], targets, chunk=chunk)
            total -= lp.double().sum()
            hits += (am == targets).sum()
            n_scored += length - first
        nll_sum, hits = float(total), int(hits)
        return {"nll_sum": nll_sum, "n_scored": n_scored, "ppl": math.exp(nll_sum / n_scored), "argmax_hits": hits}

    @torch.no_grad()
    def extend_graph(self, tokens):
        """extend() replayed from a hipGraph captured per token COUNT, with prefill_graph's cache-size rule.  The launches
        read the position on the device, so one captured graph serves every start position."""
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        if tokens.numel() < 1:
            raise ValueError("extend_graph: an empty token list")

        def warmup(static_tok):
            # on the tokens of this very call: it appends the rows the replay writes again, bit for bit; the counter goes
            # back to where it was
            pos0 = self.pos.clone()
            self.extend(static_tok)
            self.pos.copy_(pos0)
        return self._replay_per_length(self._extend_graphs, tokens, warmup, self.extend)

    # ---- speculative greedy decode (spec.py) ------------------------------------------------------------------
    def _spec_state(self):
        """the device state of a speculative decode at fixed addresses (a captured pass reads and writes it in place):
        the pass's rows, hist, the prediction buffer, the emitted tokens and the counters (csrc/spec_rows.hip.h)"""
        if self._spec is None:
            def z(n, dt=torch.long):
                return torch.zeros(n, dtype=dt, device=self.dev)
            cap = min(max(4096, 4 * self.max_len), _spec.MAX_CORPUS - (self.max_len + 1))
            self._spec = dict(rows=z(_spec.MAX_K + 1), neg=z(_spec.MAX_K + 1) - 1, hist=z(self.max_len + 1), pred=z(cap),
                              out=z(self.max_len + _spec.MAX_K + 1), out_len=z(1), stats=z(4), n_draft=z(1, torch.int32),
                              n_pred=z(1, torch.int32))
        return self._spec

    def _spec_pass(self, k, gmin, gmax, adapter=None):
        """one pass of generate_speculative: the k + 1 rows (current token, guesses) behind the position through every block
        on the chunk route, final norm and lm_head on all rows, the scoring tail (targets -1: lse and arg-max), then accept /
        emit / rewind / draft in one launch.  Nothing is read on the host."""
        S, s = self._spec_state(), self.s
        rows = S["rows"][:k + 1]

        def tail(c0, h):
            logits = F.rms_norm(h, (s.hidden,), self.final_norm, s.rms_eps) @ self.lm_head.T
            _, lse, am = torch.ops.quip_lib.nll_rows(logits, S["neg"][:k + 1])
            torch.ops.quip_lib.spec_accept_draft(am, lse, rows, S["n_draft"], self.pos, S["hist"], S["pred"], S["n_pred"],
                                                 S["out"], S["out_len"], S["stats"], gmin, gmax)
        _extend_chunks(self, "generate_speculative", rows, k + 1, None, None, tail, adapter)

    def _spec_graph(self, k, gmin, gmax, adapter):
        """the captured pass for (k, ngram, adapter tensor), captured at first use with prefill_graph's cache-size rule.  The
        warm-up runs on the live state and puts it back: the cache rows it appends are the ones the replay writes again."""
        key = (k, gmin, gmax, None if adapter is None else adapter.data_ptr())
        if key not in self._spec_graphs:
            if len(self._spec_graphs) >= self.prefill_graph_cache_size:
                self._spec_graphs.pop(next(iter(self._spec_graphs)))
            S = self._spec_state()
            live = [self.pos, S["hist"], S["rows"], S["n_draft"], S["out"], S["out_len"], S["stats"]]

            def warmup():
                saved = [t.clone() for t in live]
                self._spec_pass(k, gmin, gmax, adapter)
                for t, t0 in zip(live, saved):
                    t.copy_(t0)
            self._spec_graphs[key] = capture_graph(warmup, lambda: self._spec_pass(k, gmin, gmax, adapter))[0]
        return self._spec_graphs[key]

    @torch.no_grad()
    def generate_speculative(self, n_tokens, prompt, k=4, ngram=(1, 3), prediction=None, use_graph=True, adapter=None):
        """generate(n_tokens, prompt=prompt) for greedy decoding, the same tokens, with up to `k` guessed tokens verified per
        pass: the current token and the guesses go through the blocks as ONE chunk pass of k + 1 rows (the codes are read once
        for all of them), the longest prefix of guesses that the model's own arg-max confirms is accepted with the model's
        next token behind it, and the cache is taken back behind the rest by moving the position.  Guesses need no second
        model: they are the continuation of the most recent place where the last ngram = (gmin, gmax) tokens -- the longest
        match first -- already occurred, in `prediction` (1-D ids: what the caller expects the output to look like, as in
        editing and retrieval workloads) or in the prompt and the text generated so far; ngram = (0, 0) guesses nothing.
        quip_lib::spec_accept_draft does all of that on the device; after a pass the host reads the count of emitted tokens,
        nothing else.  use_graph: the pass is captured once per (k, ngram) and replayed at every position, whatever the
        prompt and the prediction.  Returns the (n_tokens,) ids on the device; leaves the position, the current token and
        the fed count as generate() does (generate(append=True) continues) and self.spec_stats = {passes, drafted, accepted,
        emitted}: emitted = passes + accepted >= n_tokens, the surplus of the last pass is dropped.  `adapter`: as in
        prefill().  A pass whose first row has no finite logits raises RuntimeError; nothing retries."""
        what = "generate_speculative"
        prompt = torch.as_tensor(prompt, dtype=torch.long, device=self.dev).reshape(-1)
        P, n_tokens = prompt.numel(), int(n_tokens)
        if P < 1 or n_tokens < 1:
            raise ValueError(f"{what}: prompt needs at least one token and n_tokens must be >= 1")
        if not isinstance(k, int) or not 1 <= k <= _spec.MAX_K:
            raise ValueError(f"{what}: k = {k!r} outside 1 .. {_spec.MAX_K}")
        try:
            gmin, gmax = (int(g) for g in ngram)
        except (TypeError, ValueError):
            raise ValueError(f"{what}: ngram = {ngram!r} is not a pair (gmin, gmax)") from None
        if not 0 <= gmin <= gmax <= _spec.MAX_G:
            raise ValueError(f"{what}: ngram = {ngram!r}: need 0 <= gmin <= gmax <= {_spec.MAX_G}")
        if self.sampling is not None:
            raise ValueError(f"{what}: greedy only, but a temperature is set (set_sampling(None) first)")
        if self.s.head_dim not in (64, 128):
            raise ValueError(f"{what}: head_dim {self.s.head_dim}: the chunk attention launch serves 64 and 128")
        if P - 1 + n_tokens + k > self.max_len:
            raise ValueError(f"{what}: {P} prompt tokens - 1 + n_tokens {n_tokens} + k {k} > max_len {self.max_len}: "
                             f"the last pass would not fit the cache")
        S = self._spec_state()
        n_pred = 0
        if prediction is not None:
            prediction = torch.as_tensor(prediction, dtype=torch.long, device=self.dev).reshape(-1)
            n_pred = prediction.numel()
            if n_pred > S["pred"].numel():
                raise ValueError(f"{what}: prediction of {n_pred} tokens > the buffer's {S['pred'].numel()}")
            if n_pred and not (0 <= int(prediction.min()) and int(prediction.max()) < self.s.vocab):
                raise ValueError(f"{what}: prediction holds ids outside the vocabulary 0 .. {self.s.vocab - 1}")
        self.reset()
        if P > 1:
            self.prefill(prompt[:-1], adapter=adapter)
        self.tok.copy_(prompt[-1:].view_as(self.tok))
        S["hist"][:P].copy_(prompt)
        S["rows"].zero_()
        S["rows"][:1].copy_(prompt[-1:])
        S["pred"][:n_pred].copy_(prediction if n_pred else S["pred"][:0])
        S["n_pred"].fill_(n_pred)
        for name in ("n_draft", "out_len", "stats"):
            S[name].zero_()
        torch.ops.quip_lib.spec_draft(S["rows"][:k + 1], S["n_draft"], self.pos, S["hist"], S["pred"], S["n_pred"],
                                      S["stats"], gmin, gmax)
        graph = self._spec_graph(k, gmin, gmax, adapter) if use_graph else None
        emitted = 0
        while emitted < n_tokens:
            if graph is not None:
                graph.replay()
            else:
                self._spec_pass(k, gmin, gmax, adapter)
            before, emitted = emitted, int(S["out_len"])           # the one host read of a pass
            if emitted <= before:
                break                                               # (a status bit: the pass emitted nothing)
        passes, drafted, accepted, status = S["stats"].tolist()
        if status or emitted < n_tokens:
            raise RuntimeError(f"{what}: status {status} after {passes} passes and {emitted} tokens"
                               + (": a pass gave no finite logits" if status & _spec.STATUS_NONFINITE else ""))
        out = S["out"][:n_tokens].clone()
        self.tok.copy_(out[-1:].view_as(self.tok))
        self.pos.fill_(P - 1 + n_tokens)
        self._fed = P - 1 + n_tokens
        self.spec_stats = {"passes": passes, "drafted": drafted, "accepted": accepted, "emitted": emitted}
        return out

    def reset(self, first_token=1):
        if self.block_eng and self._eng_sig != self._engine_signature():
            # a module's tensors were replaced or edited since the descriptors were baked: rebuild them (and the captured step)
            for L in self.layers:
                if hasattr(L["down"], "_eng_had3"):
                    del L["down"]._eng_had3
            self.block_eng = False
            self._init_block_engine()
            self.graph = None
        self.tok.fill_(first_token)
        self.pos.zero_()

    def capture(self):
        """warm up (kernel attribute setup, allocator: two steps) and capture one step as a hipGraph; step_logits is the
        static output of the captured step (valid after each replay)"""
        self.reset()
        self.graph, self.step_logits = capture_graph(lambda: (self.step(), self.step()), self.step)
        self.reset()

    @torch.no_grad()
    def generate(self, n_tokens, first_token=1, use_graph=True, prompt=None, temperature=None, top_k=None,
                 batched_prefill=True, prefill_graph=False, append=False):
        """decode n_tokens (greedy, or sampled when a temperature is given: set_sampling); returns the
        token ids (device tensor).  `prompt` (1-D token ids): all but its last token go through ONE batched
        pass (`prefill`; batched_prefill=False feeds them token by token through the captured step instead, teacher
        forced), then decoding continues from the last prompt token; prompt length + n_tokens <= max_len + 1.
        append=True (the next turn of a conversation; needs a `prompt`): nothing is reset -- the token the previous call
        left picked but not yet cached, then prompt[:-1], go through extend() behind what the cache holds, prompt[-1]
        becomes the current token and decoding continues.  Lengths are checked against the host-side count of the tokens
        the previous calls fed.  A step that is not captured yet runs eagerly in such a call (capturing warms up on cache
        rows 0 and 1, which the conversation still attends to)."""
        if prompt is not None:
            prompt = torch.as_tensor(prompt, dtype=torch.long, device=self.dev).reshape(-1)
            first_token = int(prompt[0]) if not append else first_token
        if append:
            fed = self._fed
            if fed is None:
                raise RuntimeError("generate(append=True): no earlier generate() call on this decoder to continue")
            if prompt is None or prompt.numel() < 1:
                raise ValueError("generate(append=True) needs a prompt of at least one token")
            if fed + prompt.numel() + n_tokens > self.max_len:
                raise ValueError(f"{fed} cached tokens + {prompt.numel()} prompt tokens + {n_tokens} new ones do not fit "
                                 f"max_len {self.max_len}")
            self.set_sampling(temperature, top_k)
            use_graph = bool(use_graph) and self.graph is not None
            out = torch.empty(n_tokens, dtype=torch.long, device=self.dev)
            self.extend(torch.cat([self.tok.reshape(1), prompt[:-1]]))
            self.tok.copy_(prompt[-1:].view_as(self.tok))
            n_prompt, pos0 = 0, fed + prompt.numel()
            return self._decode_loop(out, n_tokens, n_prompt, pos0, prompt, first_token, use_graph, True)
        n_prompt = 0 if prompt is None else prompt.numel() - 1
        assert n_prompt + n_tokens <= self.max_len
        self.set_sampling(temperature, top_k)
        self.reset(first_token)
        if use_graph and self.graph is None:
            self.capture()
            self.reset(first_token)
        out = torch.empty(n_tokens, dtype=torch.long, device=self.dev)
        if batched_prefill and n_prompt >= 1:
            # all prompt tokens but the last in one batched pass (fills cache rows 0..P-2); the last one goes through
            # the captured step like every generated token
            (self.prefill_graph if prefill_graph else self.prefill)(prompt[:-1])   # graph: captured per prompt length
            self.tok.copy_(prompt[-1:].view_as(self.tok))
            n_prompt = 0
        pos0 = prompt.numel() - 1 if (batched_prefill and prompt is not None and prompt.numel() > 1) else 0
        return self._decode_loop(out, n_tokens, n_prompt, pos0, prompt, first_token, use_graph,
                                 batched_prefill and prompt is not None and prompt.numel() > 1)

    def _decode_loop(self, out, n_tokens, n_prompt, pos0, prompt, first_token, use_graph, tok_from_prompt):
        """the token loop of generate(): n_prompt teacher-forced steps, n_tokens decoded ones, from position pos0 with the
        current token in self.tok (tok_from_prompt: that token is prompt[-1]), and the recovery from a persistent launch
        that gave up; leaves the host-side count of fed tokens for generate(append=True)"""

        replay = [bool(use_graph)]

        def run(t_from):
            for t in range(t_from, n_prompt + n_tokens):
                if replay[0]:
                    self.graph.replay()
                else:
                    self.step_logits = self.step()
                if t < n_prompt:
                    self.tok.copy_(prompt[t + 1:t + 2].view_as(self.tok))
                else:
                    out[t - n_prompt] = self.tok.reshape(-1)[0]
        run(0)
        # A persistent launch that gave up (_engine_recover) remembers the position of the first token it did not compute:
        # that token and everything behind it is decoded again -- on the stage-wise step, unless the code only said that the
        # workspace wanted zeroing (0xE000).  Cache rows of earlier positions are results.
        for _ in range(3):
            st, fail = self._engine_recover()
            if not st:
                break
            t_from = 0 if fail is None else max(0, fail - pos0)
            if use_graph and self.graph is None:
                # The rest of THIS call runs eagerly: capture() warms up with two steps at positions 0 and 1, which would
                # overwrite cache rows 0 and 1 of every layer -- rows the resumed decode still attends to.  The next
                # generate() call captures the stage-wise step (its reset + prompt pass rewrite those rows anyway).
                replay[0] = False
            self.pos.fill_(pos0 + t_from)
            if t_from == 0:
                self.tok.fill_(first_token if not tok_from_prompt else int(prompt[-1]))
            elif t_from <= n_prompt:
                self.tok.copy_(prompt[t_from:t_from + 1].view_as(self.tok))
            else:
                self.tok.copy_(out[t_from - 1 - n_prompt].view_as(self.tok))
            run(t_from)
        self._fed = pos0 + n_prompt + n_tokens
        return out
