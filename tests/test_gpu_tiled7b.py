"""The Llama-2-7B-shaped persistent launch on launch-tiled copies of the codes (csrc/decode_block_tiled.hip; codebook id 5 of
quip_block_engine; include/quip_mi355.h: quip_tile_codes_view): the layout is a pure permutation of the bytes that each weight
request fetches, so the launch computes the same bits as on the checkpoint's layout (QUIP_ENG_TILED=0), at the real n_ffn = 11008
(gate / up's row block of 11 rows, down's half slice behind the last row block)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PROJ = ("q", "k", "v", "o", "gate", "up", "down")


def _view_tile_ref(x):
    """view[j][b][c][q][n < nb(b)] = bytes [64 c + 16 q, +16) of row (16 b + n) * 256 + j, written from the index formula"""
    rows, rb = x.shape
    K, C = rows // 256, rb // 64
    out = []
    for j in range(256):
        for b in range((K + 15) // 16):
            nb = min(16, K - 16 * b)
            blk = x[(16 * b + np.arange(nb)) * 256 + j].reshape(nb, C, 4, 16)       # [n][c][q][byte]
            out.append(blk.transpose(1, 2, 0, 3).reshape(-1))                       # [c][q][n][byte]
    return np.concatenate(out)


@pytest.mark.parametrize("row_bytes", [128, 1024])
def test_view_tiler_is_the_stated_permutation_and_untile_inverts_it(row_bytes):
    from quip_for_all_amd import decode as D
    src = torch.from_numpy(np.random.default_rng(row_bytes).integers(0, 256, (11008, row_bytes), dtype=np.uint8))
    x = src.view(torch.int16).to(DEV)
    tiled = D.tile_codes_view(x)
    assert tiled.dtype == torch.uint8 and tiled.numel() == 11008 * row_bytes
    assert np.array_equal(tiled.cpu().numpy(), _view_tile_ref(src.numpy()))
    back = D.tile_codes_view(tiled.view(11008, row_bytes), inverse=True)
    assert torch.equal(back.cpu().view(11008, row_bytes), src)


def test_view_tiler_refuses_bad_shapes_misalignment_and_overlap():
    from quip_for_all_amd import capi
    L = capi.lib()
    buf = torch.zeros(4 * 256 * 64 + 64, dtype=torch.uint8, device=DEV)
    p, n = buf.data_ptr(), 256 * 64
    st = torch.cuda.current_stream().cuda_stream
    for fn in (L.quip_tile_codes_view, L.quip_untile_codes_view):
        assert fn(None, p, 256, 64, st) == -1 and fn(p, None, 256, 64, st) == -1
        assert fn(p, p + n, 255, 64, st) == -2           # rows % 256
        assert fn(p, p + n, 11008 + 16, 64, st) == -2
        assert fn(p, p + n, 256, 96, st) == -2           # row_bytes % 64
        assert fn(p, p + n, -256, 64, st) == -2
        assert fn(p + 8, p + 2 * n, 256, 64, st) == -3   # misaligned source
        assert fn(p, p + n + 8, 256, 64, st) == -3       # misaligned destination
        assert fn(p, p, 256, 64, st) == -5               # in place
        assert fn(p, p + n // 2, 256, 64, st) == -5      # partial overlap
        assert fn(p + n // 2, p, 256, 64, st) == -5
        assert fn(p, p + n, 0, 64, st) == 0              # empty: ok, no launch
        assert fn(p, p + n, 256, 64, st) == 0            # back to back: fine
    torch.cuda.synchronize()


def test_tiled_codebook_id_is_refused_on_the_other_shapes():
    """id 5 is shape 0's: the 8192-wide and the grouped-query 4096-wide launches answer QUIP_ERR_UNSUPPORTED before any launch"""
    import ctypes
    from quip_for_all_amd import capi
    L = capi.lib()
    buf = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p = buf.data_ptr()
    for shape in (1, 2):
        a = capi.BlockEngineArgs(p, p, p, p, p, p, p, p, None, 1, 16, -1, 1e-5, 0.1, 5, 0.0, shape, None)
        assert L.quip_block_engine(ctypes.byref(a), None) == -5


def _decoder(layers, tiled, max_len=48, seed=3):
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=4096, ffn=11008, layers=layers, heads=32, kv_heads=32, vocab=2048)
    old = os.environ.get("QUIP_ENG_TILED")
    os.environ["QUIP_ENG_TILED"] = "1" if tiled else "0"
    np.random.seed(1234 + seed)       # (the K x K factors come from numpy's global generator: the same model in every run)
    try:
        dec = D.LlamaDecoder(shape, "E8P12", max_len=max_len, device=DEV, seed=seed, device_init=True)
    finally:
        if old is None:
            os.environ.pop("QUIP_ENG_TILED", None)
        else:
            os.environ["QUIP_ENG_TILED"] = old
    assert dec.block_eng and dec.eng_shape == 0 and dec.eng_codebook == (5 if tiled else 0)
    return dec


def _assert_same_model(a, b):
    for La, Lb in zip(a.layers, b.layers):
        for k in PROJ:
            for name in ("Qidxs", "SU", "SV", "had_left", "had_right"):
                ta, tb = getattr(La[k], name), getattr(Lb[k], name)
                assert (ta is None) == (tb is None) and (ta is None or torch.equal(ta, tb)), (k, name)


def _forced_steps(a, b, steps=6):
    """both decoders on b's tokens: logits and the new K / V cache rows bit for bit, status 0"""
    for dec in (a, b):
        dec.reset(first_token=7)
    with torch.no_grad():
        for t in range(steps):
            la, lb = a.step().clone(), b.step().clone()
            assert a.engine_status() == 0 and b.engine_status() == 0
            assert torch.equal(la, lb), (t, (la.float() - lb.float()).abs().max().item())
            a.tok.copy_(b.tok)
    for ca, cb in ((a.kcache, b.kcache), (a.vcache, b.vcache)):
        for i in range(len(a.layers)):
            assert torch.equal(ca[i][:, :steps], cb[i][:, :steps])
            assert ca[i][:, :steps].float().abs().max().item() > 0


@pytest.mark.parametrize("layers", [1, 2])
def test_tiled_launch_equals_the_row_major_launch_bit_for_bit(layers):
    a, b = _decoder(layers, True), _decoder(layers, False)
    _assert_same_model(a, b)
    assert not hasattr(a.layers[0]["q"], "_qidxs_tiled") and a.layers[0]["q"].Qidxs is not None
    _forced_steps(a, b)


def test_codes_edited_in_place_rebuild_the_tiled_copies_on_reset():
    """`Qidxs` stays the truth: after an in-place edit reset() makes the descriptors, and with them the tiled copies, again.  The
    row-major launch reads `Qidxs` itself, so it is the decoder "built fresh with those codes" without any copy in between"""
    a, b = _decoder(1, True), _decoder(1, False)
    g = torch.Generator(device=DEV).manual_seed(11)
    with torch.no_grad():
        a.reset(first_token=7)
        before = a.step().clone()
        for k in ("gate", "down"):
            m = a.layers[0][k]
            new = torch.randint(-32768, 32768, m.Qidxs.shape, generator=g, device=DEV, dtype=torch.int32).to(m.Qidxs.dtype)
            m.Qidxs.copy_(new)
            b.layers[0][k].Qidxs.copy_(new)
    _assert_same_model(a, b)
    _forced_steps(a, b)               # (reset() inside: a's signature changed)
    with torch.no_grad():
        a.reset(first_token=7)
        assert not torch.equal(a.step(), before)       # the edit reached the launch
