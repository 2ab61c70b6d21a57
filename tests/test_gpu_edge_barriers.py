"""The 4096-wide edges of the persistent block launch (csrc/decode_block.hip, edge()) exchange through TWO buffers -- fwd through
kBuf0, rev through kBuf1, the digit planes on kBuf0 -- and execute two workgroup barriers instead of six (DESIGN 4.11 has the table
of every barrier between a gather and the next publication).  None of that is arithmetic, so these tests compare bits:
  * golden equality -- per greedy step the logits (sha256, 16 sampled values), the next token, and the appended K / V cache rows,
    against what the commit BEFORE the change computed (tests/golden/edge_barriers/golden.json, written by
    tools/edge_barriers_golden.py with that commit's library), for the three instantiations whose edges changed: the launch-tiled
    E8P12 launch, the row-major nibble launch and one byte-table codebook (D4); 1 and 2 blocks; from position 0 and from position 100
    behind a fixed history.  The straddling workgroups 85 / 170 (two consumers, two plane sets) have rows in every logit;
  * the same launch 20 times on one input: a missing barrier is a race, and a race shows as logits that differ between launches.
The kernel's shape is fixed (hidden 4096, ffn 11008): the smallest case is one full-size block.  All waits are bounded: an error is a
status code."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from tests.test_gpu_block_engine import _decoder
from tests.test_gpu_tiled7b import _decoder as _decoder_7b

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "edge_barriers", "golden.json")
BUILDS = ["tiled", "row_major", "D4"]
STEPS, TOKEN, MAX_LEN = 6, 7, 112
POSITIONS = [0, 100]
SAMPLED = [3 + 127 * i for i in range(16)]          # 16 logits spread over the 2048
PROJ = ("q", "k", "v", "o", "gate", "up", "down")


@functools.lru_cache(maxsize=None)
def _build(name, layers):
    if name in ("tiled", "row_major"):
        return _decoder_7b(layers, name == "tiled", max_len=MAX_LEN)
    dec = _decoder(layers, True, max_len=MAX_LEN, codebook=name)
    assert dec.block_eng and dec.eng_shape == 0 and dec.eng_codebook == {"D4": 1}[name]
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


def _start(dec, layers, pos0):
    """token 7 at position pos0 on a zeroed workspace; positions < pos0 hold a fixed history (numpy's PCG64: the same everywhere)"""
    dec.reset(first_token=TOKEN)
    dec.engine_reset()
    rng = np.random.Generator(np.random.PCG64(1000 + pos0))
    for i in range(layers):
        for c in (dec.kcache, dec.vcache):
            c[i].zero_()
            if pos0:
                hist = (rng.standard_normal((c[i].shape[0], pos0, c[i].shape[2])) * 0.5).astype(np.float16)
                c[i][:, :pos0].copy_(torch.from_numpy(hist))
    dec.pos.fill_(pos0)


def measure(build, layers, pos0):
    """six greedy steps from token 7 at position pos0: what every step answered, and the cache rows they appended"""
    dec = _build(build, layers)
    steps = []
    with torch.no_grad():
        _start(dec, layers, pos0)
        for t in range(STEPS):
            lg = dec.step().clone()
            assert dec.engine_status() == 0, (build, layers, pos0, t, dec.engine_status())
            assert torch.isfinite(lg).all()
            flat = lg.reshape(-1)
            steps.append({"logits_sha256": _sha(lg), "token": int(dec.tok.item()),
                          "logits16": [int(x) for x in flat[SAMPLED].cpu().view(torch.int16).numpy().view(np.uint16)]})
    rows = [c[i][:, pos0:pos0 + STEPS] for c in (dec.kcache, dec.vcache) for i in range(layers)]
    assert all(r.float().abs().max().item() > 0 for r in rows)
    return {"inputs_sha256": _inputs_fingerprint(dec), "steps": steps, "kv_rows_sha256": _sha(*rows)}


@pytest.mark.parametrize("pos0", POSITIONS)
@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("build", BUILDS)
def test_same_bits_as_before_the_change(build, layers, pos0):
    with open(GOLDEN) as f:
        want = json.load(f)["cases"][f"{build}-{layers}-{pos0}"]
    got = measure(build, layers, pos0)
    print(build, layers, pos0, got)
    assert got["inputs_sha256"] == want["inputs_sha256"], \
        "the fixture's inputs are not reproduced here (the decoder's codes / SU / SV differ from those the golden file was recorded on)"
    for t, (g, w) in enumerate(zip(got["steps"], want["steps"])):
        assert g["logits16"] == w["logits16"] and g["token"] == w["token"], (t, g["logits16"], w["logits16"])
        assert g["logits_sha256"] == w["logits_sha256"], t
    assert len(got["steps"]) == len(want["steps"]) == STEPS
    assert got["kv_rows_sha256"] == want["kv_rows_sha256"]


@pytest.mark.parametrize("build", BUILDS)
def test_twenty_launches_on_one_input_give_the_same_bits(build):
    """two blocks at position 100 (the edge between the blocks feeds products; attention over the history): the same token at the same
    position 20 times -- logits and the appended rows identical every time"""
    layers, pos0 = 2, 100
    dec = _build(build, layers)
    with torch.no_grad():
        _start(dec, layers, pos0)
        first, rows0 = None, None
        for it in range(20):
            dec.tok.fill_(TOKEN)
            dec.pos.fill_(pos0)
            lg = dec.step().clone()
            rows = torch.stack([c[i][:, pos0] for c in (dec.kcache, dec.vcache) for i in range(layers)]).clone()
            if first is None:
                first, rows0 = lg, rows
                assert dec.engine_status() == 0 and torch.isfinite(first).all()
                continue
            assert torch.equal(lg, first), (it, dec.engine_status(), (lg.float() - first.float()).abs().max().item())
            assert torch.equal(rows, rows0), it
    assert dec.engine_status() == 0
