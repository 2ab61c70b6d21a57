"""The MLP edge of the persistent block launch (csrc/decode_block.hip) hands its 11008 (G8: 14336) rows over as {2 x fp16, tag}
granules, and every workgroup loads the granules its K-mix multiplies STRAIGHT into the MFMA's A operands: twelve (G8: sixteen) 8-byte
loads per thread, each accepted on its own tag, no LDS image in between.  What that can get wrong is a protocol matter, so these
tests look at the protocol: a granule accepted on a stale tag (generation wrap), a never-written granule consumed without a tag
(owners beyond the last one, row 43 of the last owner, G8's rows from 56 on) and every instantiation that compiles the same code.
The kernel's shape is fixed: the smallest case is one or two full-size blocks.  All waits are bounded, so a protocol error shows
as a status code, never as a hang."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.test_gpu_block_engine import _decoder, _decoder_g8, _same_weights, _ulps
from tests.test_gpu_tiled7b import _decoder as _decoder_7b

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN16X2 = 0x7E007E00          # two fp16 quiet NaNs


def _build(name, layers):
    if name == "g8":
        dec = _decoder_g8(layers, True)
        assert dec.block_eng and dec.eng_shape == 2
        return dec
    return _decoder_7b(layers, name == "tiled")


def _launch_from_start(dec):
    """the token launch on token 7 at position 0"""
    dec.tok.fill_(7)
    dec.pos.zero_()
    return dec.step().clone()


@pytest.mark.parametrize("build", ["tiled", "row_major", "g8"])
def test_generation_wrap_accepts_no_stale_granule(build):
    """packed hand-offs compare a 6-bit launch generation: 130 one-block token launches on one workspace cross the wrap twice,
    every one from the same token and position -- the same logits every time, status 0"""
    dec = _build(build, 1)
    dec.reset(first_token=7)
    dec.engine_reset()
    with torch.no_grad():
        first = _launch_from_start(dec)
        assert dec.engine_status() == 0 and torch.isfinite(first).all()
        for it in range(1, 130):
            lg = _launch_from_start(dec)
            assert torch.equal(lg, first), (it, dec.engine_status(), (lg.float() - first.float()).abs().max().item())
    assert dec.engine_status() == 0
    assert int(dec.eng_ws[:4].view(torch.int32).item()) >= 130          # the launch generation: past 64 twice


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("build", ["tiled", "g8"])
def test_dead_payloads_stay_dead(build, layers):
    """the VALUE dword of every granule behind the control words poisoned with fp16 NaNs on a freshly reset workspace, the tag
    dwords untouched: a lane that consumes a never-written granule without a tag check answers NaN, a lane that waits for one
    leaves a status code.  The logits equal those of the same launch on a clean workspace."""
    dec = _build(build, layers)
    with torch.no_grad():
        dec.reset(first_token=7)
        dec.engine_reset()
        clean = _launch_from_start(dec)
        assert dec.engine_status() == 0 and torch.isfinite(clean).all()
        dec.reset(first_token=7)
        dec.engine_reset()
        gran = dec.eng_ws[64:].view(torch.int32)
        assert gran.numel() % 2 == 0
        gran[0::2] = NAN16X2
        assert int(gran[1::2].abs().max().item()) == 0
        got = _launch_from_start(dec)
        assert dec.engine_status() == 0
        assert torch.isfinite(got).all()
        assert torch.equal(got, clean), (got.float() - clean.float()).abs().max().item()


def _one_block_against_stagewise_ulps(a, b, steps=6):
    """test_gpu_block_engine.test_block_engine_against_stagewise_step's loop and bound, one block"""
    _same_weights(b, a)
    assert a.block_eng and not b.block_eng
    for dec in (a, b):
        dec.reset(first_token=7)
    worst = 0.0
    with torch.no_grad():
        for t in range(steps):
            la, lb = a.step().clone(), b.step().clone()
            assert a.engine_status() == 0 and b.engine_status() == 0
            worst = max(worst, _ulps(la, lb))
            a.tok.copy_(b.tok)
    print(f"one block: logits within {worst:.2f} fp16 ulps of rms(logits) of the stage-wise step")
    assert worst <= 2.0 * (4.0 * np.sqrt(1) + 2.0), worst


def test_e8p12_nibble_row_major_one_block():
    old = os.environ.get("QUIP_ENG_TILED")
    os.environ["QUIP_ENG_TILED"] = "0"
    try:
        a = _decoder(1, True)
    finally:
        if old is None:
            os.environ.pop("QUIP_ENG_TILED", None)
        else:
            os.environ["QUIP_ENG_TILED"] = old
    assert a.eng_codebook == 0
    _one_block_against_stagewise_ulps(a, _decoder(1, False))


def test_g8_one_block():
    _one_block_against_stagewise_ulps(_decoder_g8(1, True), _decoder_g8(1, False))


@pytest.mark.parametrize("codebook,code", [("D4", 1), ("E8P12RVQ4B", 2)])
def test_table_mode_and_virtual_rows_one_block(codebook, code):
    """D4 (the one-table mode) and one RVQ codebook (virtual rows of twice the width: twice the digits of down's input) against the
    plain stage-wise step, with test_gpu_block_engine.test_block_engine_d4_matches_stagewise's bound"""
    a = _decoder(1, True, max_len=40, codebook=codebook)
    c = _decoder(1, False, ffn_engine=False, max_len=40, codebook=codebook)
    _same_weights(c, a)
    assert a.block_eng and a.eng_codebook == code and not c.block_eng and not c.ffn_eng
    for dec in (a, c):
        dec.reset(first_token=5)
    with torch.no_grad():
        for t in range(4):
            la, lc = a.step().float().clone(), c.step().float().clone()
            assert a.engine_status() == 0
            assert (la - lc).abs().max().item() <= 2.0 ** -8 * lc.abs().max().item(), (t, (la - lc).abs().max().item())
            a.tok.copy_(c.tok)


def _byte_tables_child():
    """runs with QUIP_ENG_REP=24, QUIP_ENG_TILED=0 (read once per process): the byte-table kernels of shape 0 and of G8"""
    a = _decoder(1, True)
    assert a.eng_codebook == 0
    _one_block_against_stagewise_ulps(a, _decoder(1, False))
    _one_block_against_stagewise_ulps(_decoder_g8(1, True), _decoder_g8(1, False))
    print("byte tables ok")


def test_e8p12_byte_tables_one_block():
    """the table mode is a switch of the library that is read once per process (QUIP_ENG_REP=24): a child process"""
    env = dict(os.environ, QUIP_ENG_REP="24", QUIP_ENG_TILED="0", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_mlp_edge import _byte_tables_child as f; f()"],
                       cwd=REPO, env=env, capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0 and "byte tables ok" in r.stdout
