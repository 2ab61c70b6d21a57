"""LlamaDecoder.generate_speculative with the pass replayed from a captured graph: the same bits as the eager route
(tokens, cache rows, position, stats), one graph per k, replayed -- not captured again -- for another prompt length and
another prediction, and side by side with the decoder's captured decode step."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 128
N_TOKENS = 20


@functools.lru_cache(maxsize=None)
def _decoder(shape_name):
    from quip_for_all_amd import decode as D
    return D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=MAX_LEN, device=DEV, seed=3)


def _fresh(shape_name):
    dec = _decoder(shape_name)
    dec.reset()
    dec.kcache.zero_()
    dec.vcache.zero_()
    return dec


def _prompt(dec, n, seed):
    g = torch.Generator().manual_seed(seed)
    half = torch.randint(0, dec.s.vocab, ((n + 1) // 2,), generator=g)
    return torch.cat([half, half])[:n].to(DEV)


def _run(shape_name, use_graph, prompt, k, prediction, n=N_TOKENS):
    dec = _fresh(shape_name)
    out = dec.generate_speculative(n, prompt, k=k, prediction=prediction, use_graph=use_graph).clone()
    pos = int(dec.pos)
    return out, dec.kcache[:, :, :pos].clone(), dec.vcache[:, :, :pos].clone(), pos, int(dec.tok), dict(dec.spec_stats)


def _same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3:] == b[3:])


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_captured_pass_equals_the_eager_one_and_is_captured_once_per_k(shape_name):
    dec = _fresh(shape_name)
    dec._spec_graphs.clear()
    p1, p2 = _prompt(dec, 11, 5), _prompt(dec, 30, 6)
    eager = {k: _run(shape_name, False, p1, k, None) for k in (1, 4)}
    assert len(dec._spec_graphs) == 0
    # the true continuation (what the eager call returned) as the prediction, and a corrupted one
    truth = eager[4][0]
    wrong = torch.where(torch.arange(truth.numel(), device=DEV) % 3 == 2, (truth + 1) % dec.s.vocab, truth)
    for k in (1, 4):
        assert _same(_run(shape_name, True, p1, k, None), eager[k])            # captures, on the live state
        assert len(dec._spec_graphs) == (1 if k == 1 else 2)
    graphs = dict(dec._spec_graphs)
    for prompt, prediction in ((p1, truth), (p1, wrong), (p2, None), (p2, wrong[:7])):
        want = _run(shape_name, False, prompt, 4, prediction)
        assert _same(_run(shape_name, True, prompt, 4, prediction), want)
        assert dec._spec_graphs == graphs                                       # replayed: the same graph objects


def test_the_captured_step_survives_a_speculative_call():
    dec = _fresh("SMALL")
    prompt = _prompt(dec, 11, 5)
    first = dec.generate(8, prompt=prompt).clone()                              # captures the decode step
    assert dec.graph is not None
    step_graph = dec.graph
    spec = dec.generate_speculative(8, prompt, k=4, use_graph=True).clone()
    assert dec.graph is step_graph
    again = dec.generate(8, prompt=prompt).clone()                              # replays it
    assert torch.equal(again, first)
    assert torch.equal(dec.generate_speculative(8, prompt, k=4, use_graph=True), spec)
