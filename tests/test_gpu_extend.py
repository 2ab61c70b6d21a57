"""LlamaDecoder.extend / extend_graph / generate(append=True) and BatchDecoder.extend_slot on the device: the chunked prompt
pass that continues a live cache, against the paths that already exist (prefill from position 0, the decode step token by
token).  Different but equivalent kernels -> the project's tolerance for this comparison, 0.03 (max|ref| + 1)
(tests/test_gpu_decode.py: test_batched_prompt_prefill_matches_token_by_token); bit equality where the route is the same."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 128


def _tol(ref):
    return 0.03 * (float(ref.float().abs().max()) + 1.0)


def _close(got, ref):
    return float((got.float() - ref.float()).abs().max()) <= _tol(ref)


@functools.lru_cache(maxsize=None)
def _decoder(shape_name, window=0):
    from quip_for_all_amd import decode as D
    return D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=MAX_LEN, device=DEV, seed=3, window=window)


def _fresh(shape_name, window=0):
    dec = _decoder(shape_name, window)
    dec.reset()
    dec.kcache.zero_()
    dec.vcache.zero_()
    return dec


def _tokens(dec, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, dec.s.vocab, (n,), generator=g).to(DEV)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
@pytest.mark.parametrize("plen", [6, 45])
def test_extend_from_zero_matches_prefill(shape_name, plen):
    dec = _fresh(shape_name)
    prompt = _tokens(dec, plen, plen)
    lp = dec.prefill(prompt).clone()
    kp, vp = dec.kcache.clone(), dec.vcache.clone()
    dec = _fresh(shape_name)
    le = dec.extend(prompt, chunk=512)
    assert int(dec.pos) == plen
    assert tuple(le.shape) == (1, dec.s.vocab) and _close(le, lp)
    assert _close(dec.kcache, kp) and _close(dec.vcache, vp)
    # block 0: the same projections at the same M and the same rotation -> the same bits
    assert torch.equal(dec.kcache[0][:, :plen], kp[0][:, :plen]) and torch.equal(dec.vcache[0][:, :plen], vp[0][:, :plen])
    assert not dec.kcache[:, :, plen:].any() and not dec.vcache[:, :, plen:].any()


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_extend_in_two_calls_and_in_small_chunks_matches_prefill(shape_name):
    dec = _fresh(shape_name)
    a, b = _tokens(dec, 21, 1), _tokens(dec, 30, 2)
    lp = dec.prefill(torch.cat([a, b])).clone()
    kp, vp = dec.kcache.clone(), dec.vcache.clone()
    dec = _fresh(shape_name)
    dec.extend(a)
    assert int(dec.pos) == 21
    l2 = dec.extend(b)
    assert int(dec.pos) == 51
    assert _close(l2, lp) and _close(dec.kcache, kp) and _close(dec.vcache, vp)
    dec = _fresh(shape_name)
    l7 = dec.extend(torch.cat([a, b]), chunk=7)
    assert int(dec.pos) == 51
    assert _close(l7, lp) and _close(dec.kcache, kp) and _close(dec.vcache, vp)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_extend_after_decode_steps_matches_token_by_token(shape_name):
    dec = _fresh(shape_name)
    toks = _tokens(dec, 19, 7)
    with torch.no_grad():
        for _ in range(5):
            dec.step()
        for t in range(toks.numel()):
            dec.tok.copy_(toks[t:t + 1])
            ref = dec.step().float().clone()
    assert int(dec.pos) == 24
    dec = _fresh(shape_name)
    with torch.no_grad():
        for _ in range(5):
            dec.step()
    got = dec.extend(toks)
    assert int(dec.pos) == 24
    assert _close(got, ref)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_generate_append_continues_the_conversation(shape_name):
    dec = _fresh(shape_name)
    t1, t2, n1, n2 = _tokens(dec, 9, 11), _tokens(dec, 13, 12), 6, 5
    out1 = dec.generate(n1, prompt=t1).clone()
    out2 = dec.generate(n2, prompt=t2, append=True).clone()
    assert int(dec.pos) == 9 - 1 + n1 + 13 + n2
    seq = torch.cat([t1, out1, t2, out2])
    produced = set(range(9, 9 + n1)) | set(range(9 + n1 + 13, seq.numel()))
    dec = _fresh(shape_name)
    dec.tok.copy_(seq[:1])
    with torch.no_grad():
        for t in range(seq.numel() - 1):
            lg = dec.step().float()[0]
            dec.tok.copy_(seq[t + 1:t + 2])
            if t + 1 in produced:
                tok = int(seq[t + 1])
                assert float(lg.max() - lg[tok]) <= 0.03 * (float(lg.abs().max()) + 1.0), (t, tok)
    # what does not fit is refused on the host-side count, before anything runs
    dec._fed = MAX_LEN - 5
    with pytest.raises(ValueError, match="max_len"):
        dec.generate(2, prompt=t2, append=True)
    del dec._fed


def test_windowed_extend_matches_prefill_band_path():
    dec = _fresh("TINY", 16)
    assert dec.window == 16
    prompt = _tokens(dec, 40, 5)
    lp = dec.prefill(prompt).clone()
    kp, vp = dec.kcache.clone(), dec.vcache.clone()
    dec = _fresh("TINY", 16)
    le = dec.extend(prompt)
    assert _close(le, lp) and _close(dec.kcache, kp) and _close(dec.vcache, vp)
    dec = _fresh("TINY", 16)
    l9 = dec.extend(prompt, chunk=9)
    assert _close(l9, lp) and _close(dec.kcache, kp) and _close(dec.vcache, vp)


def test_extend_graph_serves_every_start_position():
    dec = _fresh("SMALL")
    dec._extend_graphs.clear()
    first, second, history = _tokens(dec, 8, 21), _tokens(dec, 8, 22), _tokens(dec, 37, 23)
    le = dec.extend(first).clone()
    ke, ve = dec.kcache.clone(), dec.vcache.clone()
    dec = _fresh("SMALL")
    lg = dec.extend_graph(first)                     # captures
    assert int(dec.pos) == 8
    assert torch.equal(lg, le) and torch.equal(dec.kcache, ke) and torch.equal(dec.vcache, ve)
    # the same graph at position 37
    dec = _fresh("SMALL")
    dec.extend(history)
    k0, v0 = dec.kcache.clone(), dec.vcache.clone()
    le = dec.extend(second).clone()
    ke, ve = dec.kcache.clone(), dec.vcache.clone()
    dec.kcache.copy_(k0)
    dec.vcache.copy_(v0)
    dec.pos.fill_(37)
    lg = dec.extend_graph(second)
    assert len(dec._extend_graphs) == 1              # replayed, not captured again
    assert int(dec.pos) == 45
    assert torch.equal(lg, le) and torch.equal(dec.kcache, ke) and torch.equal(dec.vcache, ve)


def test_extend_slot_leaves_the_other_slots_alone():
    dec = _fresh("SMALL")
    bd = dec.batched(3)
    prompts = [_tokens(dec, n, 30 + n) for n in (5, 12, 8)]
    for b, pr in enumerate(prompts):
        bd.fill_slot(b, pr)
    k0, v0, tok0, pos0 = bd.kcache.clone(), bd.vcache.clone(), bd.tok.clone(), bd.pos.clone()
    more = _tokens(dec, 17, 40)
    got = bd.extend_slot(1, more).clone()
    assert bd.pos.tolist() == [4, 11 + 17, 7] and torch.equal(bd.tok, tok0)
    for b in (0, 2):
        assert torch.equal(bd.kcache[:, b], k0[:, b]) and torch.equal(bd.vcache[:, b], v0[:, b])
    assert torch.equal(bd.kcache[:, 1, :, :11], k0[:, 1, :, :11]) and torch.equal(bd.vcache[:, 1, :, :11], v0[:, 1, :, :11])
    # the same on the bs = 1 decoder
    dec.prefill(prompts[1][:-1])
    ref = dec.extend(more)
    assert _close(got, ref)
    assert _close(bd.kcache[:, 1], dec.kcache) and _close(bd.vcache[:, 1], dec.vcache)
    with pytest.raises(ValueError):
        bd.extend_slot(3, more)
