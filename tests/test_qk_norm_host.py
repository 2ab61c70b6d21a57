"""The q / k norm (Qwen3) without a GPU: the C ABI of the three entry points (declared, bound, argument checks before any
launch), the ops' fakes, qk_norm_ref against HF's own Qwen3RMSNorm on the inputs of the GPU tests, LlamaShape's free
head_dim, the random-init constructor's stream, and what from_hf / the HF wrapper refuse."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("quip_qk_norm_rows_f16", "quip_rope_attn_decode_qknorm_f16", "quip_rope_attn_decode_batched_qknorm_f16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_qk_norm_entry_points(lib):
    hdr = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    assert abi >= 19
    assert lib.quip_abi_version() == abi
    from quip_for_all_amd import capi
    assert set(NEW) <= set(capi.SIGNATURES)
    for n in NEW:
        assert hasattr(lib, n)


def test_qk_norm_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def rows(*, q=p16, qw=p16, n=2, heads=4, kvh=2, hd=64):
        return lib.quip_qk_norm_rows_f16(q, p16, qw, p16, n, heads, kvh, hd, 1e-6, None)
    assert rows(q=None) == -1 and rows(qw=None) == -1
    assert rows(q=p16 + 2) == -3 and rows(qw=p16 + 8) == -3
    assert rows(n=0) == -2 and rows(heads=0) == -2 and rows(kvh=0) == -2
    assert rows(hd=96) == -5 and rows(hd=32) == -5 and rows(hd=256) == -5

    def one(*, q=p16, qw=p16, kw=p16, heads=4, kvh=2, hd=64, window=0):
        return lib.quip_rope_attn_decode_qknorm_f16(q, p16, p16, p16, p16, p16, p16, p16, p16, heads, kvh, hd, 32, 0.125,
                                                    window, None, None, qw, kw, 1e-6)
    assert one(q=None) == -1 and one(qw=None) == -1 and one(kw=None) == -1
    assert one(q=p16 + 2) == -3 and one(kw=p16 + 2) == -3
    assert one(heads=6, kvh=4) == -2 and one(window=-1) == -2
    assert one(hd=96) == -5

    def batched(*, q=p16, qw=p16, batch=3, heads=4, kvh=2, hd=64, window=0):
        return lib.quip_rope_attn_decode_batched_qknorm_f16(q, p16, p16, p16, p16, p16, p16, p16, p16, batch, heads, kvh, hd,
                                                            32, 0.125, window, None, None, qw, p16, 1e-6)
    assert batched(q=None) == -1 and batched(qw=None) == -1
    assert batched(qw=p16 + 2) == -3
    assert batched(batch=0) == -2 and batched(heads=6, kvh=4) == -2 and batched(window=-1) == -2
    assert batched(hd=96) == -5


def test_qk_norm_op_fakes_on_meta_tensors():
    import quip_for_all_amd.qk_norm  # noqa: F401  (defines the three ops)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    B, H, KVH, HD, L = 3, 8, 2, 64, 40
    f32, i64 = torch.float32, torch.int64
    assert torch.ops.quip_lib.qk_norm_rows(m(5, H * HD), m(5, KVH * HD), m(HD), m(HD), HD, 1e-6) is None
    out = torch.ops.quip_lib.rope_attn_decode_qknorm(m(H, HD), m(KVH, HD), m(KVH, HD), m(L, HD, dtype=f32), m(L, HD, dtype=f32),
                                                     m(1, dtype=i64), m(KVH, L, HD), m(KVH, L, HD), None, 0, m(HD), m(HD), 1e-6)
    assert out.device.type == "meta" and tuple(out.shape) == (H, HD) and out.dtype == torch.float16
    out = torch.ops.quip_lib.rope_attn_decode_batched_qknorm(m(B, H, HD), m(B, KVH, HD), m(B, KVH, HD), m(L, HD, dtype=f32),
                                                             m(L, HD, dtype=f32), m(B, dtype=i64), m(B, KVH, L, HD),
                                                             m(B, KVH, L, HD), None, 0, m(HD), m(HD), 1e-6)
    assert out.device.type == "meta" and tuple(out.shape) == (B, H, HD) and out.dtype == torch.float16


def test_reference_interval_holds_hf_qwen3_rmsnorm():
    """HF's Qwen3RMSNorm in fp16 on the CPU lies inside qk_norm_ref's [lo, hi] on every element of the GPU tests' inputs:
    the reference alone meets the condition the kernel is held to"""
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm
    from quip_for_all_amd.qk_norm import qk_norm_ref
    from tests.test_gpu_qk_norm import EPS, ROWS, SHAPES, norm_inputs
    open_, total = 0, 0
    for heads, kv_heads, hd in SHAPES:
        for rows in ROWS:
            q, k, qw, kw = norm_inputs(rows, heads, kv_heads, hd)
            for x, w in ((q, qw), (k, kw)):
                x = x.reshape(rows, -1, hd)
                hf = Qwen3RMSNorm(hd, eps=EPS).half()
                with torch.no_grad():
                    hf.weight.copy_(w)
                    y = hf(x)
                lo, hi = qk_norm_ref(x, w, EPS)
                assert lo.dtype == hi.dtype == torch.float16 and lo.shape == x.shape
                assert not torch.isnan(y).any() and not torch.isnan(lo).any() and not torch.isnan(hi).any()
                assert bool(((y >= lo) & (y <= hi)).all()), (heads, kv_heads, hd, rows)
                open_ += int((lo != hi).sum())
                total += lo.numel()
    print(f"qk_norm_ref: {open_} of {total} elements have lo != hi ({100.0 * open_ / total:.3f} %)")
    assert open_ < 0.05 * total          # (an interval that is open everywhere would hold anything)


def test_llama_shape_head_dim_is_optional():
    from quip_for_all_amd.decode import LLAMA2_7B, TINY, LlamaShape
    assert LlamaShape().head_dim == 128 and LLAMA2_7B.head_dim == 128 and TINY.head_dim == 64
    s = LlamaShape(hidden=256, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512)
    assert s.head_dim == 64 and s.q_width == 256 and s == TINY
    assert LlamaShape(4096, 11008, 32, 32, 32, 32000, 1e-5, 10000.0) == LLAMA2_7B          # (the positional order stands)
    s = LlamaShape(hidden=256, heads=4, head_dim=128)
    assert s.head_dim == 128 and s.q_width == 512


def _state(dec):
    out = {"embed": dec.embed, "lm_head": dec.lm_head, "final_norm": dec.final_norm}
    for i, L in enumerate(dec.layers):
        for k, v in L.items():
            if torch.is_tensor(v):
                out[f"{i}.{k}"] = v
            else:
                for n, t in list(v.named_buffers()) + list(v.named_parameters()):
                    out[f"{i}.{k}.{n}"] = t
    return out


def _build(**kw):
    from quip_for_all_amd import decode as D
    np.random.seed(11)                  # (the K x K factors come from numpy's global generator)
    return D.LlamaDecoder(kw.pop("shape", D.TINY), "E8P12", max_len=16, device="cpu", seed=3, **kw)


def test_random_init_stream_is_untouched_without_the_flag():
    a, b = _state(_build()), _state(_build(qk_norm=False))
    assert a.keys() == b.keys() and not any("norm" in k and "final" not in k for k in a)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    dec = _build(qk_norm=True)
    c = _state(dec)
    assert dec.qk_norm and set(c) - set(a) == {"0.q_norm", "0.k_norm", "1.q_norm", "1.k_norm"}
    for k in a:                        # the norm weights are drawn behind their block: everything before them is as it was
        if not k.startswith("1."):
            assert torch.equal(a[k], c[k]), k
    w = c["0.q_norm"]
    assert tuple(w.shape) == (64,) and w.dtype == torch.float16 and 0.02 < float((w.float() - 1).std()) < 0.3
    # the persistent launches, the _z attention launch and the token tail have no norm: off on such a model
    assert not dec.block_eng and not dec.attn_z and not dec._token_tail_on()


def test_free_head_dim_widens_q_and_o_only():
    from quip_for_all_amd.decode import LlamaShape
    s = LlamaShape(hidden=256, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512, head_dim=128)
    dec = _build(shape=s, qk_norm=True)
    L = dec.layers[0]
    assert (L["q"].in_features, L["q"].out_features) == (256, 512) and (L["o"].in_features, L["o"].out_features) == (512, 256)
    assert L["k"].out_features == L["v"].out_features == 256 and tuple(L["q_norm"].shape) == (128,)
    assert tuple(dec.kcache.shape) == (2, 2, 16, 128) and tuple(dec.cos.shape) == (16, 128)


class _Rms(torch.nn.Module):
    def __init__(self, n, eps=1e-6):
        super().__init__()
        self.weight = torch.nn.Parameter(1.0 + 0.1 * torch.randn(n))
        self.variance_epsilon = eps

    def forward(self, x):
        x32 = x.float()
        return (self.weight * (x32 * torch.rsqrt(x32.pow(2).mean(-1, keepdim=True) + self.variance_epsilon))).to(x.dtype)


def _hf_stub(model_type="qwen3", norm_width=64, heads=4, kv_heads=2, head_dim=64):
    """what from_hf looks at before it touches a module: config, input_layernorm, the attention's q_norm / k_norm"""
    cfg = types.SimpleNamespace(model_type=model_type, hidden_act="silu", hidden_size=256, intermediate_size=688,
                                num_hidden_layers=1, num_attention_heads=heads, num_key_value_heads=kv_heads,
                                head_dim=head_dim, rms_norm_eps=1e-6, vocab_size=320, rope_theta=10000.0)
    attn = types.SimpleNamespace(q_norm=_Rms(norm_width), k_norm=_Rms(norm_width if norm_width == head_dim else kv_heads * head_dim))
    blk = types.SimpleNamespace(input_layernorm=_Rms(256), self_attn=attn, mlp=types.SimpleNamespace())
    return types.SimpleNamespace(config=cfg, model=types.SimpleNamespace(layers=[blk]), forward=None, training=False,
                                 parameters=lambda: iter([torch.zeros(1)]))


def test_from_hf_refuses_norms_over_the_full_width_and_qwen3_moe():
    from quip_for_all_amd.decode import LlamaDecoder
    assert "qwen3" in LlamaDecoder.LLAMA_LIKE and "qwen3_moe" not in LlamaDecoder.LLAMA_LIKE
    with pytest.raises(NotImplementedError, match="head_dim"):          # OLMo2-style: a weight of heads * head_dim
        LlamaDecoder.from_hf(_hf_stub(norm_width=4 * 64), max_len=16, device="cpu")
    with pytest.raises(NotImplementedError, match="model_type"):
        LlamaDecoder.from_hf(_hf_stub(model_type="qwen3_moe"), max_len=16, device="cpu")
    # the pair itself is taken where it is an RMSNorm over head_dim, with the module's eps ...
    qn, kn, eps = LlamaDecoder._hf_qk_norm(_hf_stub().model.layers[0].self_attn, 64)
    assert eps == 1e-6 and qn.weight.numel() == kn.weight.numel() == 64
    # ... and refused where the arithmetic is another one ((1 + w) scaling, Gemma-style)
    bad = _hf_stub().model.layers[0].self_attn
    bad.q_norm.forward = lambda x, n=bad.q_norm: _Rms.forward(n, x) + _Rms.forward(n, x) / n.weight.to(x.dtype)
    with pytest.raises(NotImplementedError, match="RMSNorm"):
        LlamaDecoder._hf_qk_norm(bad, 64)
    assert LlamaDecoder._hf_qk_norm(types.SimpleNamespace(), 64) is None          # (Llama: no such modules)


def test_hf_wrapper_precheck_follows_from_hf():
    from quip_for_all_amd.hf_fast import _FastDecode
    assert "head_dim" in _FastDecode(_hf_stub(norm_width=4 * 64)).disabled
    assert "qwen3_moe" in _FastDecode(_hf_stub(model_type="qwen3_moe")).disabled
