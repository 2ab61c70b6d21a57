"""hf_fast's batch route: `enable_fast_decode(model, batch=True)` sends the decode steps of a LEFT-PADDED HF generate batch
through a padded BatchDecoder (one attention launch for all sequences, the padded cache layout kept).  Every generated
token of every row must pass the teacher-forced margin check of tests/test_gpu_batch_decode_hf.py against the stock
forward of that sequence alone, unpadded; everything the route does not vouch for stays on the stock forward with the
stock tokens."""
import pytest
import torch

pytestmark = pytest.mark.gpu
transformers = pytest.importorskip("transformers")

from tests.test_quantizer_host import _fill_random, _tiny_config   # noqa: E402

DEV = "cuda:0"
PROMPTS = ([1, 17, 42, 99, 7, 250], [5, 300], [3, 9, 200, 41, 11, 77, 150, 2, 63])      # lengths 6, 2, 9
NEW = 8


@pytest.fixture(scope="module")
def model():
    from transformers import AutoModelForCausalLM
    from quip_for_all_amd.quantizer import QuipQuantizer
    torch.manual_seed(0)
    m = AutoModelForCausalLM.from_config(_tiny_config(), dtype=torch.float16)
    QuipQuantizer(codebook="E8P12", inference=True, ft_epochs=0).convert_model(m)
    _fill_random(m, seed=3)
    m = m.to(DEV).eval()
    m.generation_config.eos_token_id = None
    m.generation_config.pad_token_id = 0
    return m


def _padded(side="left"):
    width = max(len(p) for p in PROMPTS)
    ids = torch.zeros(len(PROMPTS), width, dtype=torch.long)
    mask = torch.zeros(len(PROMPTS), width, dtype=torch.long)
    for b, p in enumerate(PROMPTS):
        sl = slice(width - len(p), width) if side == "left" else slice(0, len(p))
        ids[b, sl] = torch.tensor(p)
        mask[b, sl] = 1
    return ids.to(DEV), mask.to(DEV)


def _check_margins(model, new_tokens):
    """new_tokens (B, NEW): every token's margin under the stock forward of prompt + tokens of that sequence alone"""
    fwd = model.forward
    fd = getattr(model, "_quip_fast_decode", None)
    if fd is not None:
        model.forward = fd.orig_forward
    try:
        for b, p in enumerate(PROMPTS):
            seq = torch.cat([torch.tensor(p, device=DEV), new_tokens[b]])[None]
            with torch.no_grad():
                logits = model(seq).logits.float()[0]
            for t in range(new_tokens.shape[1]):
                row = logits[len(p) - 1 + t]
                margin = (row.max() - row[int(new_tokens[b, t])]).item()
                assert margin <= 0.03 * (row.abs().max().item() + 1.0), (b, t, margin)
    finally:
        model.forward = fwd


def test_left_padded_generate_runs_the_batched_decoder(model):
    from quip_for_all_amd.hf_fast import disable_fast_decode, enable_fast_decode
    ids, mask = _padded()
    enable_fast_decode(model, batch=True)
    try:
        fd = model._quip_fast_decode
        out = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False, return_dict_in_generate=True)
        assert fd.disabled is None and fd.batch_disabled is None, (fd.disabled, fd.batch_disabled)
        assert fd.fast_batch_steps == NEW - 1 and fd.fast_steps == 0 and fd.batch_imports == 1, \
            (fd.fast_batch_steps, fd.fast_steps, fd.batch_imports)
        new = out.sequences[:, ids.shape[1]:]
        assert tuple(new.shape) == (len(PROMPTS), NEW)
        _check_margins(model, new)
        assert out.past_key_values.get_seq_length() == ids.shape[1] + NEW - 1
        # a second generation on the same wrapper reuses the decoder and takes the new cache object over
        out2 = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False)
        assert fd.fast_batch_steps == 2 * (NEW - 1) and fd.batch_imports == 2
        _check_margins(model, out2[:, ids.shape[1]:])
        # ... and the first generation's cache object kept its rows when it lost the buffers
        k0 = out.past_key_values.layers[0].keys
        assert k0.data_ptr() != fd.bdec.kcache[0].data_ptr() and k0.shape[-2] == ids.shape[1] + NEW - 1
    finally:
        disable_fast_decode(model)


def test_by_hand_with_a_stock_step_in_the_middle(model):
    """a prompt call, then steps on a DynamicCache; one step in the middle takes the stock forward (which concatenates
    into fresh tensors), the next fast step imports again"""
    from transformers import DynamicCache
    from quip_for_all_amd.hf_fast import disable_fast_decode, enable_fast_decode
    ids, mask = _padded()
    enable_fast_decode(model, batch=True)
    try:
        fd = model._quip_fast_decode
        cache = DynamicCache(config=model.config)

        def call(tok, mask):
            pos = (mask.cumsum(-1) - 1).clamp(min=0)[:, -tok.shape[1]:]
            with torch.no_grad():
                lg = model(tok, attention_mask=mask, position_ids=pos, past_key_values=cache, use_cache=True).logits
            assert lg.shape == (len(PROMPTS), tok.shape[1], model.config.vocab_size)
            return lg[:, -1].argmax(-1, keepdim=True)
        tok = call(ids, mask)
        new = [tok]
        for i in range(NEW - 1):
            mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
            if i == 3:
                model.forward = fd.orig_forward
            tok = call(tok, mask)
            model.forward = fd
            new.append(tok)
            assert cache.get_seq_length() == ids.shape[1] + i + 1
        assert fd.fast_batch_steps == NEW - 2 and fd.batch_imports == 2 and fd.fast_steps == 0, \
            (fd.fast_batch_steps, fd.batch_imports, fd.fast_steps)
        _check_margins(model, torch.cat(new, dim=1))
    finally:
        disable_fast_decode(model)


def _hole():
    ids, mask = _padded()
    mask[2, 4] = 0                       # a hole inside the longest row
    return ids, mask


@pytest.mark.parametrize("what", ["right_padded", "hole", "batch_not_enabled"])
def test_calls_that_stay_on_the_stock_forward(model, what):
    from quip_for_all_amd.hf_fast import disable_fast_decode, enable_fast_decode
    ids, mask = {"right_padded": lambda: _padded("right"), "hole": _hole, "batch_not_enabled": _padded}[what]()
    want = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False)
    enable_fast_decode(model, batch=what != "batch_not_enabled")
    try:
        fd = model._quip_fast_decode
        got = model.generate(ids, attention_mask=mask, max_new_tokens=NEW, do_sample=False)
        assert fd.fast_batch_steps == 0 and fd.fast_steps == 0 and fd.batch_imports == 0
        assert torch.equal(got, want), (what, got, want)
    finally:
        disable_fast_decode(model)
