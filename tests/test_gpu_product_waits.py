"""The product phases of the persistent block launch (csrc/decode_block.hip) multiply weight codes that wait in registers for
requests issued one dependency edge earlier.  The gate / up products of shape 0 wait for each live item's codes on their own
(esync::wait_all_but: "all but the N requests issued behind it"), with down's requests going out between the multiplies; the other
phases wait for the whole queue.  A wait that is one request short reads a slot before its load has landed: the previous user's codes,
hence logits hundreds of ulps away -- and the more likely the slower the loads are.  So every launch (the tiled and the row-major
nibble kernels, G8, the byte tables, D4, the RVQ codebooks, HI) runs 4 greedy steps from position 0 on 2 and 3 full-size blocks
  (a) against the stage-wise step of the same model, teacher forced, within the bounds tests/test_gpu_block_engine.py states,
  (b) once more with a 512 MB device buffer overwritten before every step, so that the codes come from HBM and not from a cache:
      logits and cache rows are bit for bit those of the run without it,
  (c) with engine_status() == 0 after every step.
The kernel's widths are fixed (hidden 4096; ffn 11008, G8: 14336): two blocks are the smallest launch in which a block hands
requests over to the next one, three the smallest with a block that both receives and hands over."""
import functools
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
DEV = "cuda:0"
STEPS, MAX_LEN, FLUSH_BYTES = 4, 256, 512 << 20
OTHER_CODEBOOKS = {"D4": 1, "E8P12RVQ4B": 2, "HI": 3, "E8P12RVQ3B": 4}
BUILDS = ["tiled", "row_major", "g8"] + list(OTHER_CODEBOOKS)


def _engine(build, layers):
    if build == "g8":
        dec = _decoder_g8(layers, True, max_len=MAX_LEN)
        assert dec.block_eng and dec.eng_shape == 2
    elif build in ("tiled", "row_major"):
        dec = _decoder_7b(layers, build == "tiled", max_len=MAX_LEN)
    else:
        dec = _decoder(layers, True, max_len=MAX_LEN, codebook=build)
        assert dec.block_eng and dec.eng_codebook == OTHER_CODEBOOKS[build]
    return dec


def _stagewise(build, layers):
    """the reference of test_gpu_block_engine.py for this launch: the stage-wise step with the MLP engine (E8P12, G8) or the plain
    one (the other codebooks)"""
    if build == "g8":
        return _decoder_g8(layers, False, max_len=MAX_LEN)
    if build in ("tiled", "row_major"):
        return _decoder(layers, False, max_len=MAX_LEN)
    return _decoder(layers, False, ffn_engine=False, max_len=MAX_LEN, codebook=build)


def _rows(cache):
    """the cache rows of the positions the steps wrote, of every block"""
    if isinstance(cache, (list, tuple)):
        return torch.stack([c[:, :STEPS] for c in cache]).clone()
    return cache[:, :, :STEPS].clone()


def _steps(dec, forced=None, flush=None):
    """STEPS steps from position 0 on token 7; `forced`: the token fed after each step (else the step's own arg-max); `flush`: a
    device buffer overwritten before every step.  -> logits [STEPS, vocab], tokens [STEPS], k rows, v rows"""
    dec.reset(first_token=7)
    if getattr(dec, "block_eng", False):
        dec.engine_reset()
    logits, toks = [], []
    with torch.no_grad():
        for t in range(STEPS):
            if flush is not None:
                flush.fill_(t + 1)
            logits.append(dec.step().clone())
            assert dec.engine_status() == 0, (t, dec.engine_status())
            if forced is not None:
                dec.tok.copy_(forced[t])
            toks.append(dec.tok.clone().reshape(-1))
    return torch.stack(logits), torch.stack(toks), _rows(dec.kcache), _rows(dec.vcache)


@functools.lru_cache(maxsize=None)
def _reference(family, layers):
    """computed once per model (the tiled and the row-major launch share theirs) and left unchanged"""
    ref = _stagewise(family, layers)
    return ref, _steps(ref)


@functools.lru_cache(maxsize=None)
def _engine_runs(build, layers):
    ref, (_, rtok, _, _) = _reference("tiled" if build == "row_major" else build, layers)
    dec = _engine(build, layers)
    _same_weights(dec, ref)      # (the K x K factors of the shared reference, which stays as it is; the descriptors are rebuilt)
    assert dec.block_eng
    plain = _steps(dec, forced=rtok)
    flush = torch.empty(FLUSH_BYTES, dtype=torch.uint8, device=DEV)
    cold = _steps(dec, forced=rtok, flush=flush)
    del flush
    return plain, cold


def _check_against_stagewise(build, layers, got, ref):
    la, lb = got[0], ref[0]
    if build in OTHER_CODEBOOKS:
        for t in range(STEPS):
            d = (la[t].float() - lb[t].float()).abs().max().item()
            print(f"{build}, {layers} blocks, step {t}: max |logit difference| {d:.5f} (bound {2.0 ** -8 * lb[t].float().abs().max().item():.5f})")
            assert d <= 2.0 ** -8 * lb[t].float().abs().max().item(), (t, d)
    else:
        worst = max(_ulps(la[t], lb[t]) for t in range(STEPS))
        print(f"{build}, {layers} blocks: logits within {worst:.2f} fp16 ulps of rms(logits) of the stage-wise step (bound {2.0 * (4.0 * np.sqrt(layers) + 2.0):.1f})")
        assert worst <= 2.0 * (4.0 * np.sqrt(layers) + 2.0), worst
        for ca, cb_ in ((got[2], ref[2]), (got[3], ref[3])):
            assert (ca.float() - cb_.float()).abs().max().item() <= 2.0 ** -7 * cb_.float().abs().max().item()


def _check_cold_equals_plain(plain, cold):
    assert torch.equal(cold[0], plain[0]), (cold[0].float() - plain[0].float()).abs().max().item()
    assert torch.equal(cold[2], plain[2]) and torch.equal(cold[3], plain[3])


@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("build", BUILDS)
def test_products_wait_for_the_codes_they_multiply(build, layers):
    plain, cold = _engine_runs(build, layers)
    _check_against_stagewise(build, layers, plain, _reference("tiled" if build == "row_major" else build, layers)[1])
    _check_cold_equals_plain(plain, cold)


@pytest.mark.parametrize("layers", [2, 3])
def test_tiled_launch_equals_row_major_launch(layers):
    """the tiled layout is a permutation of the bytes each request fetches: the same bits, with either set of waits"""
    for i in (0, 1):
        t, r = _engine_runs("tiled", layers)[i], _engine_runs("row_major", layers)[i]
        assert torch.equal(t[0], r[0]) and torch.equal(t[2], r[2]) and torch.equal(t[3], r[3])


def _byte_tables_child():
    """runs with QUIP_ENG_REP=24, QUIP_ENG_TILED=0 (read once per process): the byte-table kernels of shape 0 and of G8"""
    for build in ("row_major", "g8"):
        for layers in (2, 3):
            plain, cold = _engine_runs(build, layers)
            _check_against_stagewise(build, layers, plain, _reference("tiled" if build == "row_major" else build, layers)[1])
            _check_cold_equals_plain(plain, cold)
    print("byte tables ok")


def test_byte_table_launches():
    """the table mode is a switch of the library that is read once per process (QUIP_ENG_REP=24): a child process"""
    env = dict(os.environ, QUIP_ENG_REP="24", QUIP_ENG_TILED="0", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", "from tests.test_gpu_product_waits import _byte_tables_child as f; f()"],
                       cwd=REPO, env=env, capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0 and "byte tables ok" in r.stdout
