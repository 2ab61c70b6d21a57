"""The routed sparse-MoE MLP without a GPU: the C ABI of the three launches (declared, bound, refusals before any launch), the
ops' fakes, QuantMoeMlp's construction (experts that differ are refused by field name, the modules' codes alias the stack) and
LlamaDecoder.from_hf on a tiny Mixtral-shaped model."""
import ctypes
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("quip_moe_route_rows_f16", "quip_moe_mm_skinny_f16", "quip_moe_combine_rows_f16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_entries_and_the_abi_version(lib):
    from quip_for_all_amd import capi
    hdr = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src)) and set(NEW) <= set(capi.SIGNATURES)
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    assert abi >= 29 and lib.quip_abi_version() == abi


def test_refusals_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def route(*, h=p, xs=p, start=p, rows=2, hidden=256, E=8, k=2, stacks=2, su=None):
        return lib.quip_moe_route_rows_f16(h, p, p, su, None, xs, start, p, p, rows, hidden, E, k, stacks, 1, 1e-5, None)
    assert route(h=None) == -1 and route(xs=None) == -1 and route(start=None) == -1
    assert route(h=p + 2) == -3 and route(su=p + 8) == -3 and route(start=p + 2) == -3
    assert route(rows=0) == -2 and route(hidden=260) == -2 and route(k=9, E=8) == -2 and route(stacks=3) == -2
    assert route(rows=32) == -5 and route(E=65) == -5 and route(E=16, k=9) == -5

    def mm(*, mode=0, x=p, q=(p, p), start=p, stacks=2, E=8, m=2, pairs=4, n=64, k=128):
        return lib.quip_moe_mm_skinny_f16(mode, x, (ctypes.c_void_p * 2)(*q), p, p, start, p, stacks, E, m, pairs, n, k, None)
    assert mm(mode=5) == -2 and mm(stacks=3) == -2 and mm(m=0) == -2 and mm(k=4) == -2
    assert mm(x=None) == -1 and mm(q=(p, None)) == -1 and mm(start=None) == -1
    assert mm(x=p + 2) == -3 and mm(q=(p + 8, p)) == -3
    assert all(mm(mode=c) == -5 for c in (1, 2, 3, 4))                     # only E8P12 is built
    assert mm(m=32, pairs=64) == -5 and mm(E=65) == -5 and mm(pairs=17) == -5 and mm(k=192) == -5 and mm(n=63) == -5

    def rows(*, mode=0, t=p, t2=None, pair_of=p, n=2, width=256, E=8, k=2, pairs=4):
        return lib.quip_moe_combine_rows_f16(mode, t, t2, None, None, None, None, p, p, pair_of, p, n, width, E, k, pairs, None)
    assert rows(mode=2) == -2 and rows(t=None) == -1 and rows(pair_of=None) == -1 and rows(mode=1, n=4) == -1
    assert rows(t=p + 2) == -3 and rows(width=260) == -2 and rows(n=3) == -2 and rows(mode=1, t2=p, n=2) == -2
    assert rows(n=32, pairs=64) == -5


def test_op_fakes_on_meta_tensors():
    import quip_for_all_amd.moe  # noqa: F401  (defines the three ops)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    ops, i32 = torch.ops.quip_lib, torch.int32
    xs, start, pair_of, weight = ops.moe_route_rows(m(3, 256), m(256), m(8, 256), None, None, 2, 2, True, 1e-5)
    assert (tuple(xs.shape), tuple(start.shape), tuple(pair_of.shape), tuple(weight.shape)) == ((2, 6, 256), (9,), (6,), (6,))
    assert (xs.dtype, start.dtype, pair_of.dtype, weight.dtype) == (torch.float16, i32, i32, torch.float32)
    y = ops.mm_skinny_moe(xs, [m(8, 512, 32, dtype=torch.int16)] * 2, m(2, 8, dtype=torch.float32), start, 3, 0,
                          m(256, dtype=torch.int64))
    assert tuple(y.shape) == (2, 6, 512) and y.dtype == torch.float16
    mid = ops.moe_combine_rows(y[0], y[1], None, None, None, None, start, None, None, 2, 1)
    out = ops.moe_combine_rows(m(6, 256), None, None, None, None, m(3, 256), start, pair_of, weight, 2, 0)
    assert tuple(mid.shape) == (6, 512) and tuple(out.shape) == (3, 256)


def _experts(E, hidden=256, ffn=512, codebook="E8P12"):
    from quip_for_all_amd.codebook import codebook_id
    from quip_for_all_amd.qlinear import QuantLinear
    cb = codebook_id[codebook](inference=True)
    return [(QuantLinear(hidden, ffn, cb, bias=False), QuantLinear(hidden, ffn, cb, bias=False),
             QuantLinear(ffn, hidden, cb, bias=False)) for _ in range(E)]


def test_quant_moe_mlp_stacks_once_and_refuses_by_name():
    from quip_for_all_amd.moe import QuantMoeMlp
    ex = _experts(3)
    block = types.SimpleNamespace(gate=types.SimpleNamespace(weight=torch.zeros(3, 256)), top_k=2,
                                  experts=[types.SimpleNamespace(w1=a, w3=b, w2=c) for a, b, c in ex])
    mlp = QuantMoeMlp.from_hf(block)
    assert mlp.top_k == 2 and mlp.n_experts == 3 and tuple(mlp.q_w2.shape) == (3, 256, 64)
    for i, (w1, w3, w2) in enumerate(ex):      # views of the stack: nothing resident twice
        assert w1.Qidxs.data_ptr() == mlp.q_w1[i].data_ptr() and w2.Qidxs.data_ptr() == mlp.q_w2[i].data_ptr()
        assert w3.Qidxs._base is mlp.q_w3

    def refused(change, word, E=3, top_k=2, **kw):
        ex = _experts(E, **kw)
        change(ex)
        with pytest.raises((NotImplementedError, TypeError), match=word):
            QuantMoeMlp(torch.zeros(E, 256), ex, top_k)
    refused(lambda ex: setattr(ex[1][0], "K_left", 3), "expert 1 w1 differs in K_left")
    refused(lambda ex: setattr(ex[2][2], "SV", None), "expert 2 w2 differs in SV")
    refused(lambda ex: setattr(ex[1][1], "had_right", torch.ones(2, 2)), "expert 1 w3 differs in had_right")
    refused(lambda ex: ex.__setitem__(1, _experts(1, ffn=1024)[0]), "expert 1 w1 differs in out_features")
    refused(lambda ex: None, "codebook 'D4'", codebook="D4")
    refused(lambda ex: None, "top_k", top_k=4)
    refused(lambda ex: ex.__setitem__(0, (torch.nn.Linear(256, 512),) * 3), "triples of QuantLinear")


class _Rms(torch.nn.Module):
    def __init__(self, n):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(n))

    def forward(self, x):
        return (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5) * self.weight.float()).to(x.dtype)


def _hf_mixtral(model_type="mixtral", E=4):
    from quip_for_all_amd.codebook import codebook_id
    from quip_for_all_amd.qlinear import QuantLinear
    cb = codebook_id["E8P12"](inference=True)
    ql = lambda i, o: QuantLinear(i, o, cb, bias=False)  # noqa: E731
    cfg = types.SimpleNamespace(model_type=model_type, hidden_act="silu", hidden_size=256, intermediate_size=512,
                                num_hidden_layers=1, num_attention_heads=8, num_key_value_heads=4, rms_norm_eps=1e-5,
                                vocab_size=64, rope_theta=10000.0, num_local_experts=E, num_experts_per_tok=2)
    attn = types.SimpleNamespace(q_proj=ql(256, 256), k_proj=ql(256, 128), v_proj=ql(256, 128), o_proj=ql(256, 256))
    moe = types.SimpleNamespace(gate=types.SimpleNamespace(weight=torch.zeros(E, 256)), top_k=2,
                                experts=[types.SimpleNamespace(w1=ql(256, 512), w3=ql(256, 512), w2=ql(512, 256)) for _ in range(E)])
    blk = types.SimpleNamespace(input_layernorm=_Rms(256), post_attention_layernorm=_Rms(256), self_attn=attn,
                                block_sparse_moe=moe)
    inner = types.SimpleNamespace(layers=[blk], embed_tokens=types.SimpleNamespace(weight=torch.zeros(64, 256)), norm=_Rms(256))
    return types.SimpleNamespace(config=cfg, model=inner, lm_head=types.SimpleNamespace(weight=torch.zeros(64, 256)),
                                 parameters=lambda: iter([torch.zeros(1)]))


def test_from_hf_takes_mixtral_and_still_refuses_qwen3_moe():
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.moe import QuantMoeMlp
    dec = LlamaDecoder.from_hf(_hf_mixtral(), max_len=16, device="cpu")
    assert (dec.s.n_experts, dec.s.top_k) == (4, 2) and dec.moe and isinstance(dec.layers[0]["moe"], QuantMoeMlp)
    assert "gate" not in dec.layers[0] and dec.layers[0]["moe"].top_k == 2
    assert not (dec.block_eng or dec.ffn_eng or dec.chain or dec.fused_prologue or dec.attn_z or dec._token_tail_on())
    with pytest.raises(NotImplementedError, match="enable_lora"):
        dec.enable_lora()
    with pytest.raises(NotImplementedError, match="model_type 'qwen3_moe'"):
        LlamaDecoder.from_hf(_hf_mixtral(model_type="qwen3_moe"), max_len=16, device="cpu")
    assert "mixtral" not in LlamaDecoder.LLAMA_LIKE          # (hf_fast follows LLAMA_LIKE: still off there)
