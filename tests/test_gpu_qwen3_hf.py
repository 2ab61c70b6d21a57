"""Qwen3 checkpoints (per-head q / k RMSNorm, head_dim free of hidden_size / heads) on the fast decoders: a `Qwen3Config`
model goes through QuipQuantizer.convert_model -> save -> load_quantized_model; LlamaDecoder.from_hf follows the stock HF
forward, `generate` takes the fast route on a StaticCache and on the default DynamicCache, and a left-padded batch takes
the batch route.  The pattern of tests/test_gpu_hf_generate.py: test_fast_decoder_qwen2_architecture_with_qkv_bias."""
import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

from tests.test_gpu_hf_generate import _check_prompt   # noqa: E402
from tests.test_quantizer_host import _fill_random   # noqa: E402

DEV = "cuda:0"
HEAD_DIMS = [128, 64]


def _checkpoint(tmp_path, head_dim):
    from transformers import AutoModelForCausalLM, Qwen3Config
    from quip_for_all_amd.quantizer import QuipQuantizer, load_quantized_model
    cfg = Qwen3Config(hidden_size=256, intermediate_size=688, num_hidden_layers=2, num_attention_heads=4,
                      num_key_value_heads=2, head_dim=head_dim, vocab_size=320, max_position_embeddings=64,
                      tie_word_embeddings=False)
    torch.manual_seed(4)
    model = AutoModelForCausalLM.from_config(cfg, dtype=torch.float16)
    qz = QuipQuantizer(codebook="E8P12", inference=True, ft_epochs=0)
    qz.convert_model(model)
    _fill_random(model, seed=17)
    g = torch.Generator().manual_seed(head_dim)
    with torch.no_grad():
        for blk in model.model.layers:
            for n in (blk.self_attn.q_norm, blk.self_attn.k_norm):
                assert tuple(n.weight.shape) == (head_dim,)
                n.weight.copy_((1.0 + 0.3 * torch.randn(head_dim, generator=g)).to(n.weight.dtype))
    qz.save(model, str(tmp_path))
    q = load_quantized_model(str(tmp_path), device_map={"": DEV}).eval()
    w = q.model.layers[1].self_attn.k_norm.weight
    assert q.config.model_type == "qwen3" and float((w.detach().float() - 1).abs().max()) > 0.1      # (the weights came with the checkpoint)
    assert q.model.layers[0].self_attn.q_proj.out_features == 4 * head_dim
    q.generation_config.eos_token_id = None
    q.generation_config.pad_token_id = 0
    return q


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_from_hf_follows_the_stock_forward(tmp_path, head_dim):
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.hf_fast import disable_fast_decode
    q = disable_fast_decode(_checkpoint(tmp_path, head_dim))
    dec = LlamaDecoder.from_hf(q, max_len=64)
    assert dec.qk_norm and dec.s.head_dim == head_dim and dec.s.q_width == 4 * head_dim and dec.qk_eps == q.config.rms_norm_eps
    assert tuple(dec.layers[0]["q_norm"].shape) == (head_dim,) and not dec.block_eng and not dec.attn_z
    for prompt in (torch.tensor([5, 17, 3, 99, 42], device=DEV),
                   torch.randint(0, 320, (40,), generator=torch.Generator().manual_seed(6)).to(DEV)):
        _check_prompt(q, dec, prompt)            # margin <= 0.03 (max|row| + 1) under the stock forward, 8 tokens each
    toks = dec.generate(8, prompt=prompt)
    assert torch.equal(toks, dec.generate(8, prompt=prompt, use_graph=False))


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_generate_takes_the_fast_route(tmp_path, head_dim):
    """the wrapper load_quantized_model installs: a StaticCache and the default DynamicCache decode through
    LlamaDecoder.step (fast_steps > 0); tokens as the stock route's, by the rule of the existing wrapper tests (a near tie
    may flip one of 16: at least 14 agree)"""
    from quip_for_all_amd.hf_fast import disable_fast_decode, enable_fast_decode
    q = _checkpoint(tmp_path, head_dim)
    ids = torch.tensor([[1, 17, 42, 99, 7, 250]], device=DEV)
    disable_fast_decode(q)
    want = q.generate(ids, max_new_tokens=16, do_sample=False)[0, ids.shape[1]:]
    enable_fast_decode(q)
    fd = q._quip_fast_decode
    assert fd.disabled is None, fd.disabled
    got = q.generate(ids, max_new_tokens=16, do_sample=False)[0, ids.shape[1]:]
    assert fd.disabled is None and fd.fast_steps > 0, (fd.disabled, fd.fast_steps)
    assert fd.dyn.qk_norm and fd.dyn.s.head_dim == head_dim
    assert int((got == want).sum()) >= 14, (got, want)
    steps0 = fd.fast_steps
    st = q.generate(ids, max_new_tokens=16, do_sample=False, cache_implementation="static")[0, ids.shape[1]:]
    assert fd.disabled is None and fd.fast_steps > steps0, (fd.disabled, fd.fast_steps, steps0)
    assert int((st == want).sum()) >= 14, (st, want)


@pytest.mark.parametrize("head_dim", HEAD_DIMS)
def test_left_padded_batch_takes_the_batch_route(tmp_path, head_dim):
    """enable_fast_decode(model, batch=True): the decode steps of a left-padded batch of 3 run the padded BatchDecoder
    (fast_batch_steps > 0); every generated token passes the margin check under the stock forward of its sequence alone"""
    from quip_for_all_amd.hf_fast import disable_fast_decode, enable_fast_decode
    q = disable_fast_decode(_checkpoint(tmp_path, head_dim))
    prompts = ([1, 17, 42, 99, 7, 250], [5, 300], [3, 9, 200, 41, 11, 77, 150, 2, 63])
    width, new = max(len(p) for p in prompts), 8
    ids = torch.zeros(3, width, dtype=torch.long)
    mask = torch.zeros(3, width, dtype=torch.long)
    for b, p in enumerate(prompts):
        ids[b, width - len(p):] = torch.tensor(p)
        mask[b, width - len(p):] = 1
    ids, mask = ids.to(DEV), mask.to(DEV)
    enable_fast_decode(q, batch=True)
    fd = q._quip_fast_decode
    out = q.generate(ids, attention_mask=mask, max_new_tokens=new, do_sample=False)[:, width:]
    assert fd.disabled is None and fd.batch_disabled is None, (fd.disabled, fd.batch_disabled)
    assert fd.fast_batch_steps > 0 and fd.fast_batch_steps == new - 1, fd.fast_batch_steps
    assert fd.bdec.parent.qk_norm and not fd.bdec._fuses_norm()       # (padded start: the norm launch in front)
    disable_fast_decode(q)
    for b, p in enumerate(prompts):
        seq = torch.cat([torch.tensor(p, device=DEV), out[b]])[None]
        with torch.no_grad():
            logits = q(seq).logits.float()[0]
        for t in range(new):
            row = logits[len(p) - 1 + t]
            margin = (row.max() - row[int(out[b, t])]).item()
            assert margin <= 0.03 * (row.abs().max().item() + 1.0), (b, t, margin)
