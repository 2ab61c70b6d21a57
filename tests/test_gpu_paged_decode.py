"""LlamaDecoder.batched(B, paged=True, pages=N) on the device (paged_cache.PagedBatchDecoder): given the same calls it
returns the bits of the contiguous BatchDecoder -- logits, tokens, positions and, gathered through the table, the cache
-- from a pool that is smaller than B x max_pages and was fragmented first; fork_slot shares a prefix; a pool that is
too small refuses before anything is written."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN, B = 384, 4


@functools.lru_cache(maxsize=None)
def _decoder(shape_name):
    from quip_for_all_amd import decode as D
    return D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=MAX_LEN, device=DEV, seed=3)


def _tokens(dec, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, dec.s.vocab, (n,), generator=g).to(DEV)


def _pair(shape_name, pages):
    """the contiguous decoder and the paged one on the same modules; the pool's free list out of order"""
    from quip_for_all_amd.paged_cache import PoolExhausted
    dec = _decoder(shape_name)
    ref, pg = dec.batched(B, MAX_LEN), dec.batched(B, MAX_LEN, paged=True, pages=pages)
    rng = random.Random(pages)
    order = list(range(B))
    for _ in range(3):
        rng.shuffle(order)
        for b in order:
            try:
                pg.pool.reserve(b, rng.choice(PAGE_STEPS))
            except PoolExhausted:
                pass
        rng.shuffle(order)
        for b in order:
            pg.pool.release(b)
    assert pg.pages_free() == pages and pg.pool.free != sorted(pg.pool.free, reverse=True)
    return dec, ref, pg


PAGE_STEPS = (1, 65, 130, 200)


def _same_state(ref, pg):
    assert torch.equal(pg.tok, ref.tok) and torch.equal(pg.pos, ref.pos)
    assert pg.lengths == ref.pos.tolist()
    for b, n in enumerate(pg.lengths):
        k, v = pg.gather_slot(b)
        assert torch.equal(k, ref.kcache[:, b, :, :n]) and torch.equal(v, ref.vcache[:, b, :, :n]), b
    assert pg.pool.check()


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_same_calls_same_bits(shape_name):
    dec, ref, pg = _pair(shape_name, 14)                               # 14 < 4 x 6 pages
    for d in (ref, pg):
        d.capture()
    assert pg.pages_free() == 14                                       # the borrowed pages came back
    # slot 0 at 62: the captured replays cross into a fresh page; slot 1 beyond 256: the split mode runs through pages
    prompts = [_tokens(dec, n, 10 + n) for n in (63, 270, 5, 100)]
    for d in (ref, pg):
        d.fill_slots(range(B), prompts)
    assert pg.pages_free() == 14 - (1 + 5 + 1 + 2)
    _same_state(ref, pg)
    for lists, chunk in (([_tokens(dec, 40, 20), _tokens(dec, 30, 21)], 512), ([_tokens(dec, 20, 22), _tokens(dec, 17, 23)], 16)):
        a, b = ref.extend_slots([2, 3], lists, chunk=chunk), pg.extend_slots([2, 3], lists, chunk=chunk)
        assert torch.isfinite(a).all() and torch.equal(a, b), chunk
    _same_state(ref, pg)
    more = _tokens(dec, 10, 24)
    (lp_a,), (am_a,) = ref.score_slots([3], [more])
    (lp_b,), (am_b,) = pg.score_slots([3], [more])
    assert torch.equal(lp_a.view(torch.int32), lp_b.view(torch.int32)) and torch.equal(am_a, am_b)
    _same_state(ref, pg)
    assert pg.lengths == [62, 269, 64, 156]
    for use_graph in (True, False):
        a, b = ref.decode(5, use_graph=use_graph), pg.decode(5, use_graph=use_graph)
        assert torch.equal(a, b), use_graph
        assert torch.isfinite(ref.step_logits).all() and torch.equal(ref.step_logits, pg.step_logits), use_graph
        _same_state(ref, pg)
    assert pg.lengths == [72, 279, 74, 166] and pg.pages_free() == 14 - (2 + 5 + 2 + 3)


def test_fork_shares_the_prefix():
    dec, ref, pg = _pair("TINY", 10)
    prompt = _tokens(dec, 101, 30)
    for d in (ref, pg):
        d.fill_slots([0], [prompt])
    pg.fork_slot(0, 1)
    pg.fork_slot(0, 2)
    assert 10 - pg.pages_free() == 4                                   # 2 + 2 x 1 copied, not 6
    assert pg.pool.table[1][0] == pg.pool.table[2][0] == pg.pool.table[0][0]
    for b in (1, 2):                                                   # the oracle: the slot copied with torch
        ref.kcache[:, b], ref.vcache[:, b] = ref.kcache[:, 0], ref.vcache[:, 0]
        ref.tok[b], ref.pos[b] = ref.tok[0], ref.pos[0]
    _same_state(ref, pg)
    # the forks go on, one of them past the shared page and over two more: the source keeps its bits
    k0, v0 = pg.gather_slot(0)
    lists = [_tokens(dec, 7, 31), _tokens(dec, 90, 32)]
    a, b = ref.extend_slots([1, 2], lists), pg.extend_slots([1, 2], lists)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    k1, v1 = pg.gather_slot(0)
    assert torch.equal(k0, k1) and torch.equal(v0, v1)
    _same_state(ref, pg)
    # and all three, the source too, with different continuations
    lists = [_tokens(dec, 40, 33), _tokens(dec, 3, 34), _tokens(dec, 11, 35)]
    a, b = ref.extend_slots([0, 1, 2], lists, chunk=16), pg.extend_slots([0, 1, 2], lists, chunk=16)
    assert torch.isfinite(a).all() and torch.equal(a, b)
    _same_state(ref, pg)
    assert pg.lengths[:3] == [140, 110, 201] and 10 - pg.pages_free() == 1 + 2 + 1 + 3      # the shared page once


def test_a_short_pool_refuses_before_anything_is_written():
    from quip_for_all_amd.paged_cache import PoolExhausted
    dec, ref, pg = _pair("TINY", 5)
    prompts = [_tokens(dec, 101, 40), _tokens(dec, 130, 41)]
    for d in (ref, pg):
        d.fill_slots([0, 1], prompts)
    assert pg.pages_free() == 0
    more = _tokens(dec, 40, 42)
    before = [t.clone() for t in (pg.kpool, pg.vpool, pg.table, pg.pos, pg.tok)]
    host = pg.pool.snapshot()
    with pytest.raises(PoolExhausted):
        pg.extend_slots([0], [more])
    with pytest.raises(PoolExhausted):
        pg.score_slots([0], [more])
    with pytest.raises(PoolExhausted):
        pg.fill_slots([2], [_tokens(dec, 9, 43)])
    assert all(torch.equal(a, b) for a, b in zip(before, (pg.kpool, pg.vpool, pg.table, pg.pos, pg.tok)))
    assert pg.pool.snapshot() == host and pg.pages_free() == 0
    pg.free_slot(1)
    assert pg.pages_free() == 3
    a, b = ref.extend_slots([0], [more]), pg.extend_slots([0], [more])          # the same request now succeeds
    assert torch.isfinite(a).all() and torch.equal(a, b)
    # a freed slot idles under the range rule; the live ones (0, and 2 / 3 at position 0) are the contiguous decoder's
    ref.decode(1, use_graph=False)
    pg.decode(1, use_graph=False)
    assert bool(torch.isnan(pg.step_logits[1]).all())
    for b in (0, 2, 3):
        assert torch.isfinite(ref.step_logits[b]).all() and torch.equal(pg.step_logits[b], ref.step_logits[b]), b
        assert int(pg.tok[b]) == int(ref.tok[b])
    assert pg.pool.table[1] == [-1] * pg.max_pages and pg.pages_free() == 0


def test_capture_needs_a_page_per_slot_and_generate_fills_through_the_ragged_pass():
    from quip_for_all_amd.paged_cache import PoolExhausted
    dec = _decoder("TINY")
    with pytest.raises(PoolExhausted):
        dec.batched(B, MAX_LEN, paged=True, pages=3).capture()
    ref, pg = dec.batched(B, MAX_LEN), dec.batched(B, MAX_LEN, paged=True, pages=6)
    prompts = [_tokens(dec, n, 50 + n) for n in (3, 70, 1, 20)]
    a, b = ref.generate(prompts, 4, ragged=True), pg.generate(prompts, 4)
    assert torch.equal(a, b) and pg.pages_free() == 6 - 5
