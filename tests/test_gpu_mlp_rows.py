"""The row owners of the MLP edge (csrc/decode_block.hip, "P4") take their rows from the inbox [owner][row][matrix][column] straight
into the registers of ONE wave per row, which carries the gate half and the up half side by side.  None of that is arithmetic: the
launch computes what it computed before, bit for bit.  So these tests compare bits:
  * golden equality -- logits, next token and the new cache rows of the sixth step against hashes recorded on the commit before the
    change (tests/golden/mlp_rows/golden.json, written by tools/mlp_rows_golden.py), for every instantiation of the kernel;
  * the rows that do not exist (row 43 of owner 21 at K = 43; none at K = 56) with the inbox's value dwords poisoned;
  * the pairing of a workgroup's two columns in one store: gate / up rows of the odd, then of the even columns zeroed.
The kernel's shape is fixed: the smallest case is one full-size block.  All waits are bounded: an error is a status code."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_block_engine import _decoder, _decoder_g8
from tests.test_gpu_mlp_edge import NAN16X2, _launch_from_start, _one_block_against_stagewise_ulps
from tests.test_gpu_tiled7b import _decoder as _decoder_7b

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "mlp_rows", "golden.json")
BUILDS = ["tiled", "row_major", "g8", "D4", "E8P12RVQ4B", "HI", "E8P12RVQ3B"]
STEPS, TOKEN = 6, 7
PROJ = ("q", "k", "v", "o", "gate", "up", "down")
# workspace layout (csrc/decode_block.hip): 64 bytes of control words, six vectors of 2048 granules of 8 bytes, then the inbox:
# owners x 256 columns x 2 matrices x 2 rows granules, owners = ceil(K / 2), K = 43 (n_ffn 11008) or 56 (n_ffn 14336)
INBOX_OFF = 64 + 6 * 2048 * 8


def _build(name, layers):
    if name == "g8":
        dec = _decoder_g8(layers, True)
        assert dec.block_eng and dec.eng_shape == 2
        return dec
    if name in ("tiled", "row_major"):
        return _decoder_7b(layers, name == "tiled")
    dec = _decoder(layers, True, max_len=40, codebook=name)
    assert dec.block_eng and dec.eng_codebook == {"D4": 1, "E8P12RVQ4B": 2, "HI": 3, "E8P12RVQ3B": 4}[name]
    return dec


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _inputs_fingerprint(dec):
    """sha256 of every block's codes and sign vectors, in the checkpoint's layout"""
    ts = []
    for L in dec.layers:
        for k in PROJ:
            assert L[k].Qidxs is not None
            ts += [L[k].Qidxs, L[k].SU, L[k].SV]
    return _sha(*ts)


def measure(build, layers):
    """six greedy steps from token 7 on a fresh workspace: what the sixth step left"""
    dec = _build(build, layers)
    with torch.no_grad():
        dec.reset(first_token=TOKEN)
        dec.engine_reset()
        for t in range(STEPS):
            lg = dec.step().clone()
            assert dec.engine_status() == 0, (build, layers, t, dec.engine_status())
    assert torch.isfinite(lg).all()
    rows = [c[i][:, STEPS - 1] for c in (dec.kcache, dec.vcache) for i in range(layers)]
    return {"inputs_sha256": _inputs_fingerprint(dec), "logits_sha256": _sha(lg), "kv_rows_sha256": _sha(*rows),
            "token": int(dec.tok.item()), "logits16": [int(x) for x in lg.reshape(-1)[:16].cpu().view(torch.int16).numpy().view(np.uint16)]}


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("build", BUILDS)
def test_same_bits_as_before_the_change(build, layers):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][f"{build}-{layers}"]
    got = measure(build, layers)
    print(build, layers, got)
    assert got["inputs_sha256"] == want["inputs_sha256"], \
        "the fixture's inputs are not reproduced here (the decoder's codes / SU / SV differ from those the golden file was recorded on)"
    assert got["logits16"] == want["logits16"] and got["token"] == want["token"], (got["logits16"], want["logits16"])
    assert got["logits_sha256"] == want["logits_sha256"]
    assert got["kv_rows_sha256"] == want["kv_rows_sha256"]


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("build", ["tiled", "g8"])
def test_poisoned_inbox_values_reach_no_row(build, layers):
    """ONLY the inbox's value dwords are fp16 NaN pairs, every tag zero: the wave of the row that does not exist (K = 43: the second
    row of the last owner) must hold zeros without reading them; K = 56 has no such row and must wait for every tag"""
    dec = _build(build, layers)
    owners = (56 if build == "g8" else 43) + 1 >> 1
    with torch.no_grad():
        dec.reset(first_token=TOKEN)
        dec.engine_reset()
        clean = _launch_from_start(dec)
        assert dec.engine_status() == 0 and torch.isfinite(clean).all()
        dec.reset(first_token=TOKEN)
        dec.engine_reset()
        box = dec.eng_ws[INBOX_OFF:INBOX_OFF + owners * 256 * 2 * 2 * 8].view(torch.int32)
        assert box.numel() == owners * 256 * 2 * 2 * 2
        box[0::2] = NAN16X2
        assert int(box[1::2].abs().max().item()) == 0
        got = _launch_from_start(dec)
        assert dec.engine_status() == 0
        assert torch.isfinite(got).all()
        assert torch.equal(got, clean), (got.float() - clean.float()).abs().max().item()


@pytest.mark.parametrize("parity", [1, 0])
@pytest.mark.parametrize("build", ["row_major", "g8"])
def test_column_pairs_keep_their_order(build, parity):
    """gate / up rows k * 256 + column with the column's parity zeroed in the codes: the two columns a workgroup publishes in one
    store differ systematically, so a swapped pair is hundreds of ulps off the stage-wise step"""
    if build == "g8":
        a, b = _decoder_g8(1, True), _decoder_g8(1, False)
    else:
        a, b = _decoder_7b(1, False), _decoder(1, False)
    with torch.no_grad():
        for dec in (a, b):
            for k in ("gate", "up"):
                q = dec.layers[0][k].Qidxs
                assert q.shape[0] % 256 == 0
                q[parity::2] = 0
    assert torch.equal(a.layers[0]["gate"].Qidxs, b.layers[0]["gate"].Qidxs) and torch.equal(a.layers[0]["up"].Qidxs, b.layers[0]["up"].Qidxs)
    _one_block_against_stagewise_ulps(a, b)
