"""BatchDecoder.extend_slots / fill_slots / generate(ragged=True) on the device: the ragged prompt pass that continues
several slots of a batched cache at once, against the slot-by-slot passes that already exist.  One slot is the same route
at the same M as extend_slot -> bit equality; several slots change the row count of every product (and fill_slots moves
the prompt from the SDPA route to the chunk-attention route) -> the project's tolerance for equivalent routes,
0.03 (max|ref| + 1), as in tests/test_gpu_extend.py.  Token sequences are not compared: tied fp16 logits flip greedy
tokens."""
import pytest
import torch

from tests.test_gpu_extend import MAX_LEN, _close, _decoder, _tokens, _tol

pytestmark = pytest.mark.gpu
SHAPE_NAMES = ["TINY", "SMALL"]


def _state(bd):
    return bd.kcache.clone(), bd.vcache.clone(), bd.tok.clone(), bd.pos.clone()


@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
@pytest.mark.parametrize("chunk", [512, 16])
def test_one_slot_is_extend_slot_bit_for_bit(shape_name, chunk):
    dec = _decoder(shape_name)
    hist, more = _tokens(dec, 11, 50), _tokens(dec, 45, 51)
    a, b = dec.batched(3), dec.batched(3)
    for bd in (a, b):
        bd.extend_slot(0, _tokens(dec, 5, 52))
        bd.extend_slot(1, hist)
    la = a.extend_slot(1, more, chunk=chunk).clone()
    lb = b.extend_slots([1], [more], chunk=chunk)
    assert tuple(lb.shape) == (1, dec.s.vocab) and torch.isfinite(lb).all()
    assert torch.equal(lb, la)
    assert torch.equal(b.kcache, a.kcache) and torch.equal(b.vcache, a.vcache)
    assert torch.equal(b.pos, a.pos) and b.pos.tolist() == [5, 56, 0] and torch.equal(b.tok, a.tok)


@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
@pytest.mark.parametrize("chunk", [512, 16])
def test_several_slots_against_the_slot_by_slot_loop(shape_name, chunk):
    """slots (2, 0, 3) get (4, 45, 17) tokens behind positions (0, 11, 7); slot 1 idles at position 9.  chunk 16 splits the
    45-token segment across passes and puts pieces of two segments into one pass."""
    dec = _decoder(shape_name)
    slots, lengths, behind, idle = (2, 0, 3), (4, 45, 17), (0, 11, 7), 1
    ref, bd = dec.batched(4), dec.batched(4)
    for d in (ref, bd):
        d.extend_slot(idle, _tokens(dec, 9, 60))
        for b, n in zip(slots, behind):
            if n:
                d.extend_slot(b, _tokens(dec, n, 61 + b))
    assert torch.equal(ref.kcache, bd.kcache) and torch.equal(ref.vcache, bd.vcache)
    k0, v0, tok0, pos0 = _state(bd)
    lists = [_tokens(dec, n, 70 + n) for n in lengths]
    want = torch.cat([ref.extend_slot(b, t, chunk=chunk) for b, t in zip(slots, lists)])
    got = bd.extend_slots(slots, lists, chunk=chunk)
    assert tuple(got.shape) == (3, dec.s.vocab)
    assert bd.pos.tolist() == [11 + 45, 9, 4, 7 + 17] and torch.equal(bd.pos, ref.pos)
    assert torch.equal(bd.tok, tok0) and torch.equal(bd.tok, ref.tok)
    assert torch.equal(bd.kcache[:, idle], k0[:, idle]) and torch.equal(bd.vcache[:, idle], v0[:, idle])
    for j, b in enumerate(slots):
        err = float((got[j].float() - want[j].float()).abs().max())
        print(f"{shape_name} chunk {chunk} slot {b}: logits differ by {err:.4f} (tolerance {_tol(want[j]):.4f})")
        assert _close(got[j], want[j]), (b, err)
        assert _close(bd.kcache[:, b], ref.kcache[:, b]) and _close(bd.vcache[:, b], ref.vcache[:, b]), b
        p0, p1 = int(pos0[b]), int(pos0[b]) + lengths[j]
        assert torch.equal(bd.kcache[:, b, :, :p0], k0[:, b, :, :p0]) and torch.equal(bd.vcache[:, b, :, :p0], v0[:, b, :, :p0])
        assert not bd.kcache[:, b, :, p1:].any() and not bd.vcache[:, b, :, p1:].any()
        assert bool(bd.kcache[:, b, :, p0:p1].any(dim=-1).all())                  # every row of the segment was appended


@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_fill_slots_against_the_fill_slot_loop(shape_name):
    dec = _decoder(shape_name)
    prompts = [_tokens(dec, n, 80 + n) for n in (1, 6, 45)]
    ref, bd = dec.batched(3), dec.batched(3)
    for d in (ref, bd):                               # a previous life of every slot, to be restarted
        for b in range(3):
            d.extend_slot(b, _tokens(dec, 3 + b, 90 + b))
    for b, pr in enumerate(prompts):
        ref.fill_slot(b, pr)
    bd.fill_slots([2, 0, 1], [prompts[2], prompts[0], prompts[1]])
    assert bd.pos.tolist() == [0, 5, 44] and torch.equal(bd.pos, ref.pos)
    assert torch.equal(bd.tok, ref.tok) and bd.tok.tolist() == [int(pr[-1]) for pr in prompts]
    for b, pr in enumerate(prompts):
        n = pr.numel() - 1
        if n == 0:
            continue
        assert _close(bd.kcache[:, b, :, :n], ref.kcache[:, b, :, :n]) and _close(bd.vcache[:, b, :, :n], ref.vcache[:, b, :, :n])
    with torch.no_grad():
        want, got = ref.step(), bd.step()
    assert torch.isfinite(got).all()
    for b in range(3):
        assert _close(got[b], want[b]), b
    assert torch.equal(bd.pos, ref.pos)


@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_generate_ragged(shape_name):
    dec = _decoder(shape_name)
    prompts = [_tokens(dec, n, 80 + n) for n in (1, 6, 45)]
    bd = dec.batched(3)
    n = 4
    toks = bd.generate(prompts, n, ragged=True)
    assert tuple(toks.shape) == (3, n) and toks.dtype == torch.long
    assert bool(((toks >= 0) & (toks < dec.s.vocab)).all())
    assert bd.pos.tolist() == [pr.numel() - 1 + n for pr in prompts]
    assert torch.equal(bd.tok, toks[:, -1]) and torch.isfinite(bd.step_logits).all()
    # the first token of every slot is (within the tolerance) the best one of the slot-by-slot route
    ref = dec.batched(3)
    for b, pr in enumerate(prompts):
        ref.fill_slot(b, pr)
    with torch.no_grad():
        lg = ref.step().float()
    for b in range(3):
        assert float(lg[b].max() - lg[b, toks[b, 0]]) <= _tol(lg[b]), b


@pytest.mark.parametrize("shape_name", SHAPE_NAMES)
def test_a_slot_that_does_not_fit_gets_nan_and_keeps_its_cache(shape_name):
    dec = _decoder(shape_name)
    full, bd, ref = 1, dec.batched(3), dec.batched(3)
    for d in (bd, ref):
        d.extend_slot(full, _tokens(dec, MAX_LEN - 20, 100))
        d.extend_slot(2, _tokens(dec, 7, 101))
    k0, v0, _, _ = _state(bd)
    lists = {0: _tokens(dec, 30, 102), full: _tokens(dec, 21, 103), 2: _tokens(dec, 12, 104)}
    got = bd.extend_slots([0, full, 2], [lists[0], lists[full], lists[2]])
    want = ref.extend_slots([0, 2], [lists[0], lists[2]])
    assert torch.isnan(got[1]).all()
    assert torch.equal(bd.kcache[:, full], k0[:, full]) and torch.equal(bd.vcache[:, full], v0[:, full])
    assert torch.isfinite(want).all()
    for j, b in ((0, 0), (2, 2)):
        assert _close(got[j], want[j // 2]), b
        assert _close(bd.kcache[:, b], ref.kcache[:, b]) and _close(bd.vcache[:, b], ref.vcache[:, b]), b
    # what fits exactly is served
    fits = ref.extend_slots([full], [lists[full][:20]])
    assert torch.isfinite(fits).all() and int(ref.pos[full]) == MAX_LEN
