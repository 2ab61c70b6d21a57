"""QuipQuantizer.quantize_model end to end on a small random HF Llama: the Hessians it accumulates, the model-level identity
QuantLinear(x) == nn.Linear(hatW)(x), the quality of every layer, save -> load_quantized_model -> LlamaDecoder.from_hf, and
the three calibration data forms.  One quantisation run (module fixture) serves every test."""
import copy

import numpy as np
import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")
DEV = "cuda:0"
SEQ, NSAMPLES, BATCH = 64, 16, 4


def _config():
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=688, num_hidden_layers=2, num_attention_heads=4,
                                    vocab_size=512, max_position_embeddings=128, tie_word_embeddings=False,
                                    initializer_range=0.05)


def _calibration():
    g = torch.Generator().manual_seed(11)
    return [torch.randint(0, 512, (SEQ,), generator=g) for _ in range(NSAMPLES)]


def _linears(model):
    return {name: mod for name, mod in model.named_modules() if isinstance(mod, nn.Linear) and ".layers." in name}


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """quantize_model once, with QUIP.quant and QuantLinear.pack wrapped to see the Hessians and the hatW it works with"""
    from quip_for_all_amd.qlinear import QuantLinear
    from quip_for_all_amd.quantizer import QuipQuantizer
    from quip_for_all_amd.quip import QUIP
    torch.manual_seed(5)
    np.random.seed(5)                      # the K x K orthogonal factors of 688 = 16 x 43 come from scipy's global generator
    model = transformers.AutoModelForCausalLM.from_config(_config(), dtype=torch.float16)
    original = copy.deepcopy(model)
    names = {id(mod): name for name, mod in _linears(model).items()}
    hessians, counts, hat = {}, {}, {}
    mp = pytest.MonkeyPatch()
    quant0, pack0 = QUIP.quant, QuantLinear.pack

    def quant(self, *a, **kw):
        hessians[names[id(self.layer)]] = self.H.detach().cpu().numpy().copy()
        counts[names[id(self.layer)]] = self.nsamples
        return quant0(self, *a, **kw)

    def pack(self, linear, attr):
        hat[names[id(linear)]] = linear.weight.data.detach().float().cpu().clone()
        return pack0(self, linear, attr)

    mp.setattr(QUIP, "quant", quant)
    mp.setattr(QuantLinear, "pack", pack)
    save_dir = str(tmp_path_factory.mktemp("quantized"))
    qz = QuipQuantizer(codebook="E8P12", dataset=_calibration(), nsamples=NSAMPLES, model_seqlen=SEQ, batch_size=BATCH,
                       quip_tune_iters=1, ft_epochs=0)
    try:
        qmodel = qz.quantize_model(model, None, save_dir)
    finally:
        mp.undo()
    return {"original": original, "qmodel": qmodel.to(DEV), "hessians": hessians, "counts": counts, "hat": hat,
            "save_dir": save_dir, "quantizer": qz}


def test_every_linear_was_quantised(run):
    from quip_for_all_amd.qlinear import QuantLinear
    want = set(_linears(run["original"]))
    assert len(want) == 14 and set(run["hessians"]) == want and set(run["hat"]) == want
    assert not _linears(run["qmodel"])
    assert sum(isinstance(m, QuantLinear) for m in run["qmodel"].modules()) == 14
    q = run["qmodel"]
    assert q.is_quantized and q.config.quantization_config == run["quantizer"].to_dict() and q.config.use_cache
    assert q.dtype == torch.float16 and isinstance(q.lm_head, nn.Linear)
    assert not any(m.training for m in q.modules())               # the new modules too: the kernels' forward, not the dense one


def test_hessians_are_those_of_the_original_model(run):
    """H of every linear = 2 / N sum x x^T over the calibration tokens, x the ORIGINAL model's input to that linear (blocks
    are quantised after their outputs were taken) and N the number of sequences, as QUIP.add_batch counts.  The other side
    is computed here with forward hooks on an untouched fp32 copy, in float64.  Allowed difference: float64 rounding of the
    two summation orders, 1e-9 relative to sqrt(H_ii H_jj), the size of the entry's terms (an entry that cancels to
    nearly zero has no digits of its own to compare)."""
    ref = copy.deepcopy(run["original"]).float().to(DEV).eval()
    sums = {name: torch.zeros(mod.in_features, mod.in_features, dtype=torch.float64, device=DEV)
            for name, mod in _linears(ref).items()}
    handles = []
    for name, mod in _linears(ref).items():
        def hook(_, inp, out, name=name):
            x = inp[0].detach().reshape(-1, inp[0].shape[-1]).double()
            sums[name] += x.T @ x
        handles.append(mod.register_forward_hook(hook))
    ids = torch.stack(_calibration())
    with torch.no_grad():
        for lo in range(0, NSAMPLES, BATCH):
            part = ids[lo:lo + BATCH].to(DEV)
            ref(input_ids=part, attention_mask=torch.ones_like(part), use_cache=False)
    for h in handles:
        h.remove()
    for name, S in sums.items():
        assert run["counts"][name] == NSAMPLES
        want = (2.0 / NSAMPLES * S).cpu().numpy()
        got = run["hessians"][name]
        scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
        worst = float((np.abs(got - want) / scale).max())
        assert worst <= 1e-9, (name, worst)


def test_model_level_identity_and_quality(run):
    """the quantised model against a copy of the original with every hatW in its nn.Linear: logits on 8 fresh tokens within
    the round-trip tolerance of tests/test_gpu_quantize.py, once per linear on the path, summed; every hatW within the
    E8P12 bound of W"""
    ref = copy.deepcopy(run["original"]).float()
    for name, mod in _linears(ref).items():
        W = mod.weight.data
        rel = ((run["hat"][name] - W).norm() / W.norm()).item()
        assert rel < 0.55, (name, rel)
        mod.weight.data = run["hat"][name].clone()
    ref = ref.to(DEV).eval()
    tokens = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(23)).to(DEV)
    with torch.no_grad():
        want = ref(input_ids=tokens).logits.float()
        got = run["qmodel"](input_ids=tokens).logits.float()
    tol = 14 * (4e-3 * want.abs().max().item() + 2e-3)
    err = (got - want).abs().max().item()
    assert err <= tol, (err, tol)
    with torch.no_grad():          # ... and the original model is not what it computes: the check above can tell
        far = (run["original"].to(DEV)(input_ids=tokens).logits.float() - want).abs().max().item()
    run["original"].cpu()
    assert far > err


def test_save_load_round_trip_and_fast_decoder(run):
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.quantizer import load_quantized_model
    loaded = load_quantized_model(run["save_dir"], device_map={"": DEV})
    tokens = torch.randint(0, 512, (1, 8), generator=torch.Generator().manual_seed(29)).to(DEV)
    with torch.no_grad():
        a = run["qmodel"](input_ids=tokens).logits
        b = loaded(input_ids=tokens).logits
    assert torch.equal(a, b)
    dec = LlamaDecoder.from_hf(loaded, max_len=64)
    prompt = tokens[0, :4]
    toks = dec.generate(8, prompt=prompt, use_graph=False)
    seq = torch.cat([prompt, toks])[None]
    with torch.no_grad():
        logits = loaded(seq).logits.float()[0]
    decided = 0
    for t in range(8):
        row = logits[prompt.numel() - 1 + t]
        tol = 0.03 * (row.abs().max().item() + 1.0)           # the margin of tests/test_gpu_batch_decode_hf.py
        top2 = row.topk(2).values
        if (top2[0] - top2[1]).item() > tol:
            decided += 1
            assert int(toks[t]) == int(row.argmax()), t
        assert (row.max() - row[int(toks[t])]).item() <= tol, t
    assert decided >= 1


class _Tok:
    def __call__(self, text):
        return {"input_ids": [int(w) for w in text.split()]}


def test_data_forms_give_the_same_first_block_inputs(run):
    from quip_for_all_amd.quantizer import QuipQuantizer, calibration_batches, calibration_samples
    rows = _calibration()[:8]
    forms = {"tensors": (rows, None), "lists": ([r.tolist() for r in rows], None),
             "dicts": ([{"input_ids": r} for r in rows], None),
             "strings": ([" ".join(str(int(v)) for v in r) for r in rows], _Tok())}
    model = copy.deepcopy(run["original"])
    captured = {}
    for form, (dataset, tok) in forms.items():
        qz = QuipQuantizer(codebook="E8P12", dataset=dataset, nsamples=8, model_seqlen=SEQ, batch_size=BATCH, ft_epochs=0)
        batches = calibration_batches(calibration_samples(dataset, tok, SEQ), 8, BATCH)
        captured[form] = qz.capture_first_block_inputs(model, batches, torch.device(DEV))
        assert model.dtype == torch.float16 and next(model.parameters()).device.type == "cpu"      # left as it was
    hidden0, kwargs0 = captured["tensors"]
    assert len(hidden0) == 2 and tuple(hidden0[0].shape) == (BATCH, SEQ, 256) and hidden0[0].dtype == torch.float32
    assert hidden0[0].device.type == "cpu"                                                         # cache_on_gpu=False
    emb = run["original"].model.embed_tokens.weight.float()
    assert torch.equal(hidden0[0], emb[torch.stack(rows[:BATCH])])
    assert any(k.startswith("position") for k in kwargs0[0])

    def same(a, b):
        if isinstance(a, torch.Tensor):
            return isinstance(b, torch.Tensor) and torch.equal(a, b)
        if isinstance(a, (tuple, list)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return a == b or (a is None and b is None) or type(a) is type(b)
    for form in ("lists", "dicts", "strings"):
        hidden, kwargs = captured[form]
        assert all(torch.equal(a, b) for a, b in zip(hidden, hidden0)), form
        for kw, kw0 in zip(kwargs, kwargs0):
            assert set(kw) == set(kw0) and all(same(kw[k], kw0[k]) for k in kw), form
