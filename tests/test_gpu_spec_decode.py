"""LlamaDecoder.generate_speculative on the device, the eager route.  Exact against existing code only: a reference loop on
score() runs the same launches at the same row count with ONE real row per pass (the current token and k zeros, the position
taken back by k), so by the project's rule that a row's bits depend on that row alone the speculative
call must return the same ids and leave the same cache rows, position and current token, whatever was guessed.  Exact for the
trace: drafting is a function of tokens only, so spec.accept_draft_ref replayed on the host over the reference's tokens gives
the passes, the drafted and the accepted counts.  And within the project's tolerance for a comparison across different
kernels against the decode step (tests/test_gpu_extend.py: test_generate_append_continues_the_conversation)."""
import dataclasses
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 128
N_TOKENS = 24
KS = (1, 4, 7)
NGRAM = (1, 3)


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


def _prompt(shape_name, n=11, seed=5):
    """half as many random tokens, twice: the text repeats, so the lookup finds something without a prediction"""
    vocab = _decoder(shape_name).s.vocab
    g = torch.Generator().manual_seed(seed)
    half = torch.randint(0, vocab, ((n + 1) // 2,), generator=g)
    return torch.cat([half, half])[:n].to(DEV)


@functools.lru_cache(maxsize=None)
def _reference(shape_name, k, plen=11, n=N_TOKENS + max(KS)):
    """the reference loop on score(), n tokens (more than a call asks for: the last pass of a call may look ahead) ->
    (ids as a list, keys, values)"""
    dec = _fresh(shape_name)
    prompt = _prompt(shape_name, plen)
    dec.prefill(prompt[:-1])
    tok, neg, out = prompt[-1:], torch.full((k + 1,), -1, device=DEV), []
    for _ in range(n):
        _, am = dec.score(torch.cat([tok, torch.zeros(k, dtype=torch.long, device=DEV)]), targets=neg)
        tok = am[:1].clone()
        dec.pos -= k
        out.append(int(tok))
    return out, dec.kcache.clone(), dec.vcache.clone()


def _prediction(shape_name, k, source):
    if source == "none":
        return None
    ids = list(_reference(shape_name, k)[0])
    if source == "corrupted":
        vocab = _decoder(shape_name).s.vocab
        ids = [(t + 1) % vocab if i % 3 == 2 else t for i, t in enumerate(ids)]
    return torch.tensor(ids, device=DEV)


def _simulate(prompt, truth, n_tokens, k, ngram, prediction):
    """the trace of a call on the host: spec.accept_draft_ref driven by the true continuation `truth` (the model's arg-max
    behind any prefix of prompt ++ truth is the next token of it) -> the final stats [passes, drafted, accepted, 0], emitted"""
    from quip_for_all_amd.spec import accept_draft_ref
    seq, P = list(prompt) + list(truth), len(prompt)
    st = dict(rows_tok=[prompt[-1]] + [0] * k, n_draft=0, pos=P - 1, hist=list(prompt) + [0] * (MAX_LEN + 1 - P),
              pred=[] if prediction is None else prediction.tolist(), out=[0] * (MAX_LEN + 16), out_len=0, stats=[0, 0, 0, 0])
    st = accept_draft_ref(st, None, None, k, *ngram)
    while st["out_len"] < n_tokens:
        p0 = st["pos"]
        argmax = []
        for i in range(k + 1):                              # row i is a row of the true text as long as the guesses were
            ok = all(st["rows_tok"][j] == seq[p0 + j] for j in range(i + 1))
            argmax.append(seq[p0 + i + 1] if ok else -1)
        st["pos"] = p0 + k + 1
        st = accept_draft_ref(st, argmax, [0.0] * (k + 1), k, *ngram)
    assert st["out"][:n_tokens] == list(truth[:n_tokens])
    return st["stats"], st["out_len"]


@pytest.mark.parametrize("source", ["none", "truth", "corrupted"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_same_tokens_cache_and_trace_as_the_score_loop(shape_name, k, source):
    truth, kref, vref = _reference(shape_name, k)
    prediction = _prediction(shape_name, k, source)
    prompt = _prompt(shape_name)
    dec = _fresh(shape_name)
    out = dec.generate_speculative(N_TOKENS, prompt, k=k, ngram=NGRAM, prediction=prediction, use_graph=False)
    pos = prompt.numel() - 1 + N_TOKENS
    assert out.dtype == torch.long and tuple(out.shape) == (N_TOKENS,) and out.device == torch.device(DEV)
    assert out.tolist() == truth[:N_TOKENS]
    assert int(dec.pos) == pos and dec._fed == pos and int(dec.tok) == truth[N_TOKENS - 1]
    assert torch.equal(dec.kcache[:, :, :pos], kref[:, :, :pos]) and torch.equal(dec.vcache[:, :, :pos], vref[:, :, :pos])
    stats, emitted = _simulate(prompt.tolist(), truth, N_TOKENS, k, NGRAM, prediction)
    got = dec.spec_stats
    assert [got["passes"], got["drafted"], got["accepted"]] == stats[:3] and got["emitted"] == emitted
    assert got["emitted"] == got["passes"] + got["accepted"] >= N_TOKENS
    if source == "truth":
        # from the second pass on the text ends in a token of the prediction, whose continuation is the model's own: the
        # trace is not the trivial one (a property of the test's inputs, taken from the host simulation)
        assert stats[2] > 0 and stats[0] < N_TOKENS


def _teacher_forced_within_tolerance(shape_name, seq, produced):
    dec = _fresh(shape_name)
    dec.tok.copy_(seq[:1])
    with torch.no_grad():
        for t in range(seq.numel() - 1):
            lg = dec.step().float()[0]
            dec.tok.copy_(seq[t + 1:t + 2])
            if t + 1 in produced:
                tok = int(seq[t + 1])
                assert float(lg.max() - lg[tok]) <= 0.03 * (float(lg.abs().max()) + 1.0), (t, tok)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_tokens_within_tolerance_of_the_decode_step_and_append_continues(shape_name):
    dec = _fresh(shape_name)
    t1, n1, n2 = _prompt(shape_name), 14, 5
    t2 = _prompt(shape_name, 13, seed=12)
    out1 = dec.generate_speculative(n1, t1, k=4, ngram=NGRAM, prediction=_prediction(shape_name, 4, "corrupted"),
                                    use_graph=False).clone()
    out2 = dec.generate(n2, prompt=t2, append=True).clone()
    assert int(dec.pos) == 11 - 1 + n1 + 13 + n2
    seq = torch.cat([t1, out1, t2, out2])
    produced = set(range(11, 11 + n1)) | set(range(11 + n1 + 13, seq.numel()))
    _teacher_forced_within_tolerance(shape_name, seq, produced)


@pytest.mark.parametrize("k", [1, 4])
def test_a_pass_that_ends_exactly_at_max_len(k):
    plen = 100
    n = MAX_LEN - (plen - 1) - k                            # the largest n_tokens the call takes
    truth, kref, vref = _reference("TINY", k, plen, n)
    prompt = _prompt("TINY", plen)
    dec = _fresh("TINY")
    # no drafting: every pass emits one token, so the last one starts at plen - 1 + n - 1 and its k + 1 rows end at max_len
    out = dec.generate_speculative(n, prompt, k=k, ngram=(0, 0), use_graph=False)
    pos = plen - 1 + n
    assert out.tolist() == truth and int(dec.pos) == pos == MAX_LEN - k
    assert dec.spec_stats == {"passes": n, "drafted": 0, "accepted": 0, "emitted": n}
    assert torch.equal(dec.kcache[:, :, :pos], kref[:, :, :pos]) and torch.equal(dec.vcache[:, :, :pos], vref[:, :, :pos])
    with pytest.raises(ValueError, match="max_len"):
        dec.generate_speculative(n + 1, prompt, k=k, use_graph=False)


def test_refusals():
    dec = _fresh("TINY")
    prompt = _prompt("TINY")
    for kw, match in ((dict(k=0), "k"), (dict(k=16), "k"), (dict(k=2.5), "k"), (dict(ngram=(2, 1)), "ngram"),
                      (dict(ngram=(0, 9)), "ngram"), (dict(ngram=(-1, 2)), "ngram"), (dict(ngram=3), "ngram"),
                      (dict(n_tokens=MAX_LEN - 10 - 4 + 1), "max_len"), (dict(n_tokens=0), "n_tokens"),
                      (dict(prediction=torch.tensor([1, dec.s.vocab])), "prediction"),
                      (dict(prediction=torch.tensor([-1, 3])), "prediction")):
        args = {"n_tokens": 8, "prompt": prompt, "k": 4, "use_graph": False, **kw}
        with pytest.raises(ValueError, match=match):
            dec.generate_speculative(**args)
    with pytest.raises(ValueError, match="prompt"):
        dec.generate_speculative(8, prompt[:0], use_graph=False)
    dec.set_sampling(0.8, 5)
    try:
        with pytest.raises(ValueError, match="temperature"):
            dec.generate_speculative(8, prompt, use_graph=False)
    finally:
        dec.set_sampling(None)
    shape = dec.s
    dec.s = dataclasses.replace(shape, head_dim=32)
    try:
        with pytest.raises(ValueError, match="head_dim"):
            dec.generate_speculative(8, prompt, use_graph=False)
    finally:
        dec.s = shape
    # nothing ran: the decoder still serves
    assert dec.generate_speculative(8, prompt, k=4, use_graph=False).tolist() == _reference("TINY", 4)[0][:8]


def test_adapters_ride_on_the_pass():
    """enable_lora: the pass hands _block the sequence's adapter as extend() and score() do -- the decoder's own by default,
    `adapter` where given -- so the call equals the score() loop under the same adapter bit for bit"""
    from quip_for_all_amd import decode as D
    from tests.test_lora_host import config, make_adapter
    s, k, n = D.TINY, 4, 12
    kv = s.kv_heads * s.head_dim
    dims = {"q": (s.hidden, s.q_width), "k": (s.hidden, kv), "v": (s.hidden, kv), "o": (s.q_width, s.hidden),
            "gate": (s.hidden, s.ffn), "up": (s.hidden, s.ffn), "down": (s.ffn, s.hidden)}
    dec = D.LlamaDecoder(s, "E8P12", max_len=MAX_LEN, device=DEV, seed=3)
    dec.enable_lora(max_adapters=2, max_rank=16)
    dec.load_adapter("a", make_adapter(dims, s.layers, 16, tuple(dims), seed=100, amp=0.2), config(16, tuple(dims)))
    prompt = _prompt("TINY")

    def reference():
        dec.reset()
        dec.prefill(prompt[:-1])
        tok, neg, out = prompt[-1:], torch.full((k + 1,), -1, device=DEV), []
        for _ in range(n):
            _, am = dec.score(torch.cat([tok, torch.zeros(k, dtype=torch.long, device=DEV)]), targets=neg)
            tok = am[:1].clone()
            dec.pos -= k
            out.append(int(tok))
        return out, dec.kcache.clone(), dec.vcache.clone()
    dec.set_adapter("a")
    truth, kref, vref = reference()
    pos = prompt.numel() - 1 + n
    for explicit in (False, True):
        dec.set_adapter(None if explicit else "a")
        adapter = torch.tensor([dec.lora.index("a")], dtype=torch.int32, device=DEV) if explicit else None
        out = dec.generate_speculative(n, prompt, k=k, prediction=torch.tensor(truth, device=DEV), use_graph=False,
                                       adapter=adapter)
        assert out.tolist() == truth and int(dec.pos) == pos
        assert torch.equal(dec.kcache[:, :, :pos], kref[:, :, :pos]) and torch.equal(dec.vcache[:, :, :pos], vref[:, :, :pos])
    dec.set_adapter(None)
    plain, kplain, _ = reference()
    assert not torch.equal(kplain[:, :, :pos], kref[:, :, :pos])           # the adapter mattered
