"""The public path of batched decode: a checkpoint loaded with load_quantized_model, LlamaDecoder.from_hf(model).batched(B),
ragged prompts decoded together; every sequence follows the stock HF forward of that sequence alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

from tests.test_quantizer_host import _fill_random, _tiny_config   # noqa: E402


def test_batched_decoder_from_loaded_hf_model(tmp_path):
    from transformers import AutoModelForCausalLM
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.quantizer import QuipQuantizer, load_quantized_model
    torch.manual_seed(1)
    model = AutoModelForCausalLM.from_config(_tiny_config(), dtype=torch.float16)
    qz = QuipQuantizer(codebook="E8P12", inference=True, ft_epochs=0)
    qz.convert_model(model)
    _fill_random(model, seed=9)
    qz.save(model, str(tmp_path))
    q = load_quantized_model(str(tmp_path), device_map={"": "cuda:0"})
    bd = LlamaDecoder.from_hf(q, max_len=64).batched(3)
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(0, 320, (n,), generator=g).cuda() for n in (5, 1, 12)]
    toks = bd.generate(prompts, 8)
    assert tuple(toks.shape) == (3, 8)
    for prompt, ptoks in zip(prompts, toks):
        # the teacher-forced margin check of test_gpu_hf_generate._check_prompt, on this sequence alone
        seq = torch.cat([prompt, ptoks])[None]
        with torch.no_grad():
            logits = q(seq).logits.float()[0]
        for t in range(8):
            row = logits[prompt.numel() - 1 + t]
            margin = (row.max() - row[int(ptoks[t])]).item()
            assert margin <= 0.03 * (row.abs().max().item() + 1.0), (t, margin)
