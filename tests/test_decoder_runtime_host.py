"""LlamaDecoder's single-copy borrow without a GPU: `_row_major` lends a block's modules row-major code matrices and takes them
back whatever happens inside, and what the engine descriptors are judged by (`_engine_signature`) never sees the loan."""
import types

import pytest
import torch


def _shell(monkeypatch):
    """a decoder shell (no model, no device) of two blocks whose modules hold tiled codes only"""
    from quip_for_all_amd import decode as D

    def module(rows, cols):
        return types.SimpleNamespace(Qidxs=None, _qidxs_tiled=torch.arange(rows * cols * 2, dtype=torch.int32).to(torch.uint8),
                                     _qidxs_meta=((rows, cols), torch.int16), SU=torch.ones(4), SV=torch.ones(4),
                                     had_left=None, had_right=None, wscale_float=0.5)
    dec = D.LlamaDecoder.__new__(D.LlamaDecoder)
    dec.single_copy, dec.dev, dec._rm_scratch = True, torch.device("cpu"), {}
    dec.layers = [dict(ln1=torch.ones(4), ln2=torch.ones(4), **{k: module(16, 32 + 32 * i) for i, k in enumerate(D.PROJECTIONS)})
                  for _ in range(2)]

    def untile_on_cpu(tiled, rows, row_bytes, out):      # (the layout does not matter here: who holds which tensor does)
        assert tiled.numel() == rows * row_bytes == out.numel() * out.element_size()
        out.view(torch.uint8).reshape(-1).copy_(tiled)
        return out
    monkeypatch.setattr(D, "untile_codes", untile_on_cpu)
    return D, dec


def test_row_major_borrow_is_handed_back_and_the_signature_never_sees_it(monkeypatch):
    D, dec = _shell(monkeypatch)
    tiled = [[L[k]._qidxs_tiled for k in D.PROJECTIONS] for L in dec.layers]
    before = dec._engine_signature()
    for L in dec.layers:
        with dec._row_major(L):
            for k in D.PROJECTIONS:                           # (a) lent: a tensor of the recorded shape and dtype
                q = L[k].Qidxs
                assert torch.is_tensor(q) and (tuple(q.shape), q.dtype) == L[k]._qidxs_meta
                assert torch.equal(q.view(torch.uint8).reshape(-1), L[k]._qidxs_tiled)
            assert dec._engine_signature() == before          # (c) inside
        assert all(L[k].Qidxs is None for k in D.PROJECTIONS)
    # (b) an exception inside the `with` (an operator failing mid-block) hands everything back too
    with pytest.raises(RuntimeError, match="mid-block"):
        with dec._row_major(dec.layers[1]):
            assert all(dec.layers[1][k].Qidxs is not None for k in D.PROJECTIONS)
            raise RuntimeError("mid-block")
    assert all(L[k].Qidxs is None for L in dec.layers for k in D.PROJECTIONS)
    assert dec._engine_signature() == before                  # (c) after
    # (d) the tiled copies -- the only true copy of the weights -- are the same objects throughout
    assert all(L[k]._qidxs_tiled is t for L, ts in zip(dec.layers, tiled) for k, t in zip(D.PROJECTIONS, ts))


def test_a_failing_untile_hands_back_what_was_already_lent(monkeypatch):
    D, dec = _shell(monkeypatch)
    good = D.untile_codes

    def fails_on_the_fourth(tiled, rows, row_bytes, out):
        if tiled is dec.layers[0]["o"]._qidxs_tiled:
            raise RuntimeError("untile failed")
        return good(tiled, rows, row_bytes, out)
    monkeypatch.setattr(D, "untile_codes", fails_on_the_fourth)
    with pytest.raises(RuntimeError, match="untile failed"):
        with dec._row_major(dec.layers[0]):
            pytest.fail("the body must not run on a half-lent block")
    assert all(dec.layers[0][k].Qidxs is None for k in D.PROJECTIONS)


def test_two_copy_decoders_lend_nothing(monkeypatch):
    D, dec = _shell(monkeypatch)
    dec.single_copy = False
    with dec._row_major(dec.layers[0]):
        assert all(dec.layers[0][k].Qidxs is None for k in D.PROJECTIONS)
    assert dec._rm_scratch == {}
