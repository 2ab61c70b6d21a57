"""LlamaDecoder.batched(B, paged=True, kv_dtype="fp8") on the device (paged_cache.PagedBatchDecoder on pools of e4m3fn
bytes).  Against the fp16 paged decoder given the same calls -- and the fp16 decoder's tokens wherever the two could
diverge --: the same page accounting, layer-0 pool bytes that are the CPU oracle of the fp16 decoder's layer-0 rows
(they depend on token and position only), logits within a measured distance.  On its own: chunking, captured replays
and forked slots keep giving identical bits (the round-trip rule), and a short pool refuses before anything is written."""
import functools
import random

import numpy as np
import pytest
import torch

from tests.test_gpu_decode import _ulps_of_rms
from tests.test_gpu_paged_decode import B, MAX_LEN, PAGE_STEPS, _decoder, _tokens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ("TINY", "SMALL")
CHOICES = ("default", "suggested")            # kv_exp: all 0, or PagedBatchDecoder.suggest_kv_exp of the prompts
PROMPTS = (63, 270, 5, 100)
# Distance from the fp16 paged decoder's logits on the same teacher-forced calls, in fp16 ulps of rms(logits): twice the
# maxima observed on the MI355X (profiles/fp8_kv_bench.txt), the convention of the model-level bounds in
# test_gpu_decode.py.  (The three mantissa bits of K and V, not a few fp16 roundings, set this scale.  Arg-max agreement
# is printed, not asserted: random-init models have near-ties.)  The maxima below are from a run of this file alone; in a
# run of the whole suite the random-init models come out of another generator state: 254.50 / 252.00 / 224.38 / 225.45.
_OBSERVED = {("TINY", "default"): 364.45, ("TINY", "suggested"): 363.17, ("SMALL", "default"): 269.50, ("SMALL", "suggested"): 276.00}


def _fragment(pg, pages):
    """the pool's free list out of order (as test_gpu_paged_decode._pair does)"""
    from quip_for_all_amd.paged_cache import PoolExhausted
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
    return pg


def _fp8(dec, pages, kv_exp=None):
    return _fragment(dec.batched(B, MAX_LEN, paged=True, pages=pages, kv_dtype="fp8", kv_exp=kv_exp), pages)


def _raw(pg):
    return [pg.gather_slot_raw(b) for b in range(B)]


def _same_bytes(a, b):
    return all(torch.equal(ka, kb) and torch.equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


@functools.lru_cache(maxsize=None)
def _run(shape_name, choice):
    """the calls of test_gpu_paged_decode.test_same_calls_same_bits on an fp16 paged and an fp8 paged decoder -> what
    the tests below compare: per phase the host state of both, the logits of both, and the decoders themselves"""
    dec = _decoder(shape_name)
    prompts = [_tokens(dec, n, 10 + n) for n in PROMPTS]
    kv_exp = None
    if choice == "suggested":
        kv_exp = dec.batched(B, MAX_LEN, paged=True, pages=14).suggest_kv_exp(range(B), prompts)
    ref = _fragment(dec.batched(B, MAX_LEN, paged=True, pages=14), 14)
    f8 = _fp8(dec, 14, kv_exp)
    states, logits = [], {"ref": [], "f8": []}

    def mark(what):
        states.append((what, [(d.lengths, d.pages_free(), [list(r) for r in d.pool.table], d.pool.check()) for d in (ref, f8)]))
    for d in (ref, f8):
        d.capture()
    mark("capture")
    for d in (ref, f8):
        d.fill_slots(range(B), prompts)
    mark("fill")
    for lists, chunk in (([_tokens(dec, 40, 20), _tokens(dec, 30, 21)], 512), ([_tokens(dec, 20, 22), _tokens(dec, 17, 23)], 16)):
        for key, d in (("ref", ref), ("f8", f8)):
            logits[key].append(d.extend_slots([2, 3], lists, chunk=chunk).float().cpu())
        mark(f"extend chunk {chunk}")
    more = _tokens(dec, 10, 24)
    scores = [d.score_slots([3], [more]) for d in (ref, f8)]
    mark("score")
    for use_graph in (True, False):
        for _ in range(5):
            f8.tok.copy_(ref.tok)                             # teacher forcing: the fp16 decoder's tokens
            for key, d in (("ref", ref), ("f8", f8)):
                d.decode(1, use_graph=use_graph)
                logits[key].append(d.step_logits.float().cpu())
        mark(f"decode graph {use_graph}")
    torch.cuda.synchronize()
    return dict(dec=dec, ref=ref, f8=f8, states=states, logits=logits, scores=scores, kv_exp=f8.kv_exp)


@pytest.mark.parametrize("shape_name", SHAPES)
@pytest.mark.parametrize("choice", CHOICES)
def test_same_calls_same_accounting(shape_name, choice):
    r = _run(shape_name, choice)
    ref, f8 = r["ref"], r["f8"]
    assert f8.kpool.dtype == torch.uint8 and f8.kpool.shape == ref.kpool.shape                     # the same pages
    assert f8.kpool.numel() * f8.kpool.element_size() * 2 == ref.kpool.numel() * ref.kpool.element_size()   # half the bytes
    for what, (a, b) in r["states"]:
        assert a == b, what                                   # lengths, pages_free(), tables; pool.check() held
    assert r["states"][-1][1][1][0] == [72, 279, 74, 166] and f8.pages_free() == 14 - (2 + 5 + 2 + 3)
    assert torch.equal(f8.table, ref.table) and torch.equal(f8.pos, ref.pos)
    for x in r["logits"]["f8"] + r["logits"]["ref"]:
        assert bool(torch.isfinite(x).all())
    (lp,), _ = r["scores"][1]
    assert bool(torch.isfinite(lp).all())


@pytest.mark.parametrize("shape_name", SHAPES)
@pytest.mark.parametrize("choice", CHOICES)
def test_layer_0_bytes_are_the_cpu_oracle_of_the_fp16_rows(shape_name, choice):
    from quip_for_all_amd.paged_attn import dequant_f8, quant_f8
    r = _run(shape_name, choice)
    ke, ve = r["kv_exp"][0]
    for b in range(B):
        k16, v16 = r["ref"].gather_slot(b)
        k8, v8 = r["f8"].gather_slot_raw(b)
        assert k8.dtype == torch.uint8 and k8.shape == k16.shape
        assert torch.equal(k8[0].cpu(), quant_f8(k16[0].cpu(), ke)), b
        assert torch.equal(v8[0].cpu(), quant_f8(v16[0].cpu(), ve)), b
        # gather_slot: the values the bytes mean
        kd, vd = r["f8"].gather_slot(b)
        assert kd.dtype == torch.float16
        for i, (e_k, e_v) in enumerate(r["kv_exp"]):
            assert torch.equal(kd[i].cpu().view(torch.int16), dequant_f8(k8[i].cpu(), e_k).view(torch.int16))
            assert torch.equal(vd[i].cpu().view(torch.int16), dequant_f8(v8[i].cpu(), e_v).view(torch.int16))


@pytest.mark.parametrize("shape_name", SHAPES)
@pytest.mark.parametrize("choice", CHOICES)
def test_distance_from_the_fp16_decoder(shape_name, choice):
    r = _run(shape_name, choice)
    worst, agree, rows = 0.0, 0, 0
    for a, b in zip(r["logits"]["f8"], r["logits"]["ref"]):
        for x, y in zip(a.double().numpy(), b.double().numpy()):
            worst = max(worst, _ulps_of_rms(x, y))
            agree += int(np.argmax(x) == np.argmax(y))
            rows += 1
    print(f"fp8 paged vs fp16 paged logits, {shape_name}, kv_exp {choice} {r['kv_exp']}: max {worst:.2f} fp16 ulps of rms(logits), "
          f"arg-max agreement {agree} / {rows}")
    assert worst <= 2 * _OBSERVED[(shape_name, choice)], worst


def test_chunking_and_captured_replays_keep_the_bits():
    """extend_slots(chunk=16) against chunk=512, then captured against eager steps: identical logits and pool bytes.
    The token lists (20 and 9 rows) make chunk=16 two passes of 16 and 13 rows -- the first list is split between two
    launches, whose second finds rows in the cache that the single 29-row pass of chunk=512 takes from its inputs: the
    round-trip rule -- while every pass stays within 2 .. 31 rows.  Beyond 31 rows a pass takes another product path
    (QuantLinear.regime), whose results differ in the last bits from the small-batch path's: a property of the products
    that the fp16 decoders share (measured: with lists of 75 and 33 rows the fp16 paged decoder's logits differ by
    2.9e-3 between the two chunk sizes), so longer lists cannot show anything about the cache."""
    dec = _decoder("TINY")
    prompts = [_tokens(dec, n, 10 + n) for n in PROMPTS]
    lists = [_tokens(dec, 20, 60), _tokens(dec, 9, 61)]
    out = []
    for chunk, use_graph in ((16, True), (512, False)):
        pg = _fp8(dec, 14, [[-3, -2], [-4, 1]])
        pg.capture()
        pg.fill_slots(range(B), prompts)
        lg = pg.extend_slots([2, 3], lists, chunk=chunk)
        raw = _raw(pg)
        toks = pg.decode(4, use_graph=use_graph)
        torch.cuda.synchronize()
        out.append((lg, raw, toks, pg.step_logits.clone(), _raw(pg)))
    (la, ea, ta, sa, ra), (lb, eb, tb, sb, rb) = out
    assert torch.isfinite(la).all() and torch.isfinite(sa).all()
    assert torch.equal(la, lb) and _same_bytes(ea, eb)                  # chunk 16 == chunk 512
    assert torch.equal(ta, tb) and torch.equal(sa, sb) and _same_bytes(ra, rb)      # captured == eager


def test_fork_shares_the_prefix_and_continues_like_its_source():
    dec = _decoder("TINY")
    pg = _fp8(dec, 10)
    pg.fill_slots([0], [_tokens(dec, 101, 30)])
    pg.fork_slot(0, 1)
    pg.fork_slot(0, 2)
    assert 10 - pg.pages_free() == 4                                   # 2 + 2 x 1 copied, not 6
    assert pg.pool.table[1][0] == pg.pool.table[2][0] == pg.pool.table[0][0]
    src = pg.gather_slot_raw(0)
    for b in (1, 2):
        assert _same_bytes([pg.gather_slot_raw(b)], [src])
    assert pg.pool.check()
    # the forks go on, one of them past the shared page and over two more: the source keeps its bytes
    lists = [_tokens(dec, 7, 31), _tokens(dec, 90, 32)]
    assert torch.isfinite(pg.extend_slots([1, 2], lists)).all()
    assert _same_bytes([pg.gather_slot_raw(0)], [src])
    # the source and a fresh fork of it continue with the same tokens: the same logits, the same bytes
    pg.fork_slot(0, 3)
    same = _tokens(dec, 40, 33)
    lg = pg.extend_slots([0, 3, 1], [same, same, _tokens(dec, 3, 34)], chunk=16)
    assert torch.isfinite(lg).all() and torch.equal(lg[0], lg[1])
    assert _same_bytes([pg.gather_slot_raw(0)], [pg.gather_slot_raw(3)])
    assert pg.lengths == [140, 110, 190, 140] and pg.pool.check()
    assert 10 - pg.pages_free() == 1 + 2 + 1 + 2 + 2                   # the shared first page once
    assert pg.pool.table[3][0] == pg.pool.table[0][0]


def test_a_short_pool_refuses_before_anything_is_written():
    from quip_for_all_amd.paged_cache import PoolExhausted
    dec = _decoder("TINY")
    pg = _fp8(dec, 5)
    pg.fill_slots([0, 1], [_tokens(dec, 101, 40), _tokens(dec, 130, 41)])
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
    assert torch.isfinite(pg.extend_slots([0], [more])).all()           # the same request now succeeds
    pg.decode(1, use_graph=False)
    assert bool(torch.isnan(pg.step_logits[1]).all())                   # a freed slot idles under the range rule
    for b in (0, 2, 3):
        assert torch.isfinite(pg.step_logits[b]).all(), b


def test_generate_and_suggested_exponents():
    dec = _decoder("TINY")
    prompts = [_tokens(dec, n, 50 + n) for n in (3, 70, 1, 20)]
    pg = dec.batched(B, MAX_LEN, paged=True, pages=6, kv_dtype="fp8")
    a = pg.generate(prompts, 4)
    assert len(a) == B and pg.pages_free() == 6 - 5
    # suggest_kv_exp: per layer and K | V the smallest exponent at which the fp16 cache of these prompts fits below 448
    exps = pg.suggest_kv_exp(range(B), prompts)
    assert pg.pages_free() == 6 - 5                                      # (a scratch decoder did the work)
    ref = dec.batched(B, MAX_LEN, paged=True, pages=6)
    ref.fill_slots(range(B), [torch.cat([p, p[-1:]]) for p in prompts])  # all of the prompt cached
    assert len(exps) == dec.s.layers
    for i, (ke, ve) in enumerate(exps):
        for e, pool in ((ke, ref.kpool[i]), (ve, ref.vpool[i])):
            amax = float(pool.float().abs().max())
            assert -8 <= e <= 7 and (amax * 2.0 ** -e <= 448 or e == 7) and (amax * 2.0 ** -(e - 1) > 448 or e == -8), (i, e, amax)
