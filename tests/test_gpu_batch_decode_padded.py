"""LlamaDecoder.batched(B, padded=True) on the GPU: a BatchDecoder whose slots begin at cache row start[b] (the layout of a
left-padded HF generate batch; quip_lib::rope_attn_decode_batched_start).  With start = 0 it is the plain batched decoder
bit for bit, eager and captured; with shifted rows (NaN below start) every step's logits follow the plain decoder's
within the project's tolerance for equivalent routes -- the walk begins at start, so keys fall into other lane groups and
the merge order differs; bits may differ."""
import numpy as np
import pytest
import torch

from tests.test_gpu_decode import _ulps_of_rms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ["TINY", "SMALL"]              # the two smallest model shapes of tests/test_gpu_batch_decode.py
LENGTHS = (5, 9, 17)
STEPS = 6


def _decoder(shape_name):
    from quip_for_all_amd import decode as D
    np.random.seed(11)
    return D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=64, device=DEV, seed=3)


def _prompts(vocab, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).to(DEV) for n in LENGTHS]


def _filled(bd, prompts):
    """snapshot of a plain batched decoder after its prompt passes: (tok, pos, kcache, vcache)"""
    bd.reset()
    for b, pr in enumerate(prompts):
        bd.fill_slot(b, pr)
    return bd.tok.clone(), bd.pos.clone(), bd.kcache.clone(), bd.vcache.clone()


def _load(bd, snap, starts=(0, 0, 0)):
    """put a plain decoder's state into bd with sequence b's rows moved up by starts[b]; NaN below (padded decoders)"""
    tok, pos, kc, vc = snap
    bd.tok.copy_(tok)
    if not any(starts):
        bd.pos.copy_(pos)
        bd.kcache.copy_(kc)
        bd.vcache.copy_(vc)
    else:
        bd.kcache.zero_()
        bd.vcache.zero_()
        for b, s in enumerate(starts):
            n = int(pos[b])
            bd.kcache[:, b, :, :s] = float("nan")
            bd.vcache[:, b, :, :s] = float("nan")
            bd.kcache[:, b, :, s:s + n] = kc[:, b, :, :n]
            bd.vcache[:, b, :, s:s + n] = vc[:, b, :, :n]
        bd.pos.copy_(pos + torch.tensor(starts, device=DEV))
    if bd.start is not None:
        bd.start.copy_(torch.tensor(starts, device=DEV))


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("shape_name", SHAPES)
def test_zero_start_equals_the_plain_batched_decoder(shape_name):
    """logits, tokens, positions and caches over 6 steps, eager and captured (the captured step reads start in place)"""
    dec = _decoder(shape_name)
    plain, padded = dec.batched(3), dec.batched(3, padded=True)
    assert plain.start is None and padded.start.dtype == torch.int64 and tuple(padded.start.shape) == (3,)
    plain.capture()
    padded.capture()
    snap = _filled(plain, _prompts(dec.s.vocab, seed=2))
    for use_graph in (False, True):
        for bd in (plain, padded):
            _load(bd, snap)
        with torch.no_grad():
            for t in range(STEPS):
                if use_graph:
                    plain.graph.replay()
                    padded.graph.replay()
                    la, lb = plain.step_logits, padded.step_logits
                else:
                    la, lb = plain.step(), padded.step()
                what = (use_graph, t)
                assert torch.equal(_bits(la), _bits(lb)), what
                assert torch.equal(plain.tok, padded.tok) and torch.equal(plain.pos, padded.pos), what
        assert torch.equal(_bits(plain.kcache), _bits(padded.kcache)), use_graph
        assert torch.equal(_bits(plain.vcache), _bits(padded.vcache)), use_graph
        assert int(padded.start.abs().sum()) == 0
    padded.start.fill_(3)
    padded.reset()
    assert int(padded.start.abs().sum()) == 0 and int(padded.pos.abs().sum()) == 0


@pytest.mark.parametrize("shape_name", SHAPES)
def test_shifted_rows_follow_the_plain_decoder(shape_name):
    """starts (0, 3, 11): the plain decoder's cache rows copied up by start[b] with NaN below, pos = length + start; teacher
    forced, every step's logits within 0.03 (max|ref| + 1) of the plain decoder's; the appended rows land at pos"""
    dec = _decoder(shape_name)
    plain, padded = dec.batched(3), dec.batched(3, padded=True)
    starts = (0, 3, 11)
    snap = _filled(plain, _prompts(dec.s.vocab, seed=5))
    _load(padded, snap, starts)
    forced = torch.randint(0, dec.s.vocab, (3, STEPS), generator=torch.Generator().manual_seed(8)).to(DEV)
    worst = 0.0
    with torch.no_grad():
        for t in range(STEPS):
            ref, got = plain.step().float(), padded.step().float()
            assert torch.isfinite(got).all(), t
            for b in range(3):
                d = (got[b] - ref[b]).abs().max().item()
                assert d <= 0.03 * (ref[b].abs().max().item() + 1.0), (t, b, d)
                worst = max(worst, _ulps_of_rms(got[b].double().cpu().numpy(), ref[b].double().cpu().numpy()))
            assert torch.equal(padded.pos, plain.pos + torch.tensor(starts, device=DEV)), t
            for bd in (plain, padded):
                bd.tok.copy_(forced[:, t])
    print(f"{shape_name}: padded vs plain batched decoder, starts {starts}: max {worst:.2f} fp16 ulps of rms(logits)")
    # the rows the steps appended: finite, at pos - STEPS .. pos - 1 of every slot, nothing below start touched
    for b, s in enumerate(starts):
        p = int(padded.pos[b])
        assert torch.isfinite(padded.kcache[:, b, :, s:p]).all() and torch.isfinite(padded.vcache[:, b, :, s:p]).all()
        assert torch.isnan(padded.kcache[:, b, :, :s]).all() and torch.isnan(padded.vcache[:, b, :, :s]).all()
        assert int(padded.kcache[:, b, :, p:].abs().sum()) == 0


def test_prompt_side_methods_raise_and_paged_is_refused():
    dec = _decoder("TINY")
    bd = dec.batched(2, padded=True)
    for call in (lambda: bd.fill_slot(0, [1, 2]), lambda: bd.extend_slot(0, [1]), lambda: bd.prefill_slot(0, [1, 2]),
                 lambda: bd.fill_slots([0], [[1, 2]]), lambda: bd.extend_slots([0], [[1]]),
                 lambda: bd.score_slots([0], [[1, 2]]), lambda: bd.generate([[1], [2]], 2, use_graph=False)):
        with pytest.raises(NotImplementedError, match="padded=True"):
            call()
    with pytest.raises(ValueError, match="padded"):
        dec.batched(2, paged=True, padded=True)
