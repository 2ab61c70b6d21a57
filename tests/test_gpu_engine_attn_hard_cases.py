"""The attention phases of the persistent launches (csrc/decode_block.hip, decode_block_g8.hip, decode_block_gqa.hip) on
histories that are not 0.5 * randn.  These launches walk the cache their own way -- every nparts-th position per workgroup,
lane groups striding over those, two rounds in flight, the parts' states merged through a hand-off -- and are compared
with the stage-wise step only through the logits, so the histories are made to show in the logits:

    counted keys   K cache = 0 (every cached key scores 0), V cache = 0 but for ONE row per KV head and block, which holds
                   +-M.  The head's output is that row's weight times M: a position the walk loses or visits twice moves
                   the logits by far more than the bound (shown first, on the stage-wise decoder alone: the same planting
                   without one head's row moves its logits by >= 10 bounds; M is raised until it does, never the bound).
                   The planted rows sweep over every position below pos0 (pos0 <= 300), or over 64 positions that include
                   0, pos0 - 1 and every residue of 8 and of the lane-group count (pos0 = 1021).
    sharp history  K cache = 4 * randn (scores of tens of units, the running maximum moves), V cache = 0.5 * randn.

The bounds are those of each launch's own long-context test (fp16 ulps of rms(logits): 16 for the 7B launch, 18 for G8, 20
for the 8192-wide one; block 0's new cache rows as there), on the same positions.

What was observed on an MI355X is in the tests' docstrings and in profiles/attn_hard_cases.txt."""
import functools

import pytest
import torch

from tests import test_gpu_block_engine as E7
from tests import test_gpu_block_engine_gqa as EG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FAMILIES = {
    # make(engine), same_weights(engine decoder, stage-wise decoder), logits bound, bound of block 0's new rows
    "7b": (lambda eng: E7._decoder(2, eng, max_len=1100), lambda a, b: E7._same_weights(b, a), 16.0, 2.0 ** -8),
    "g8": (lambda eng: E7._decoder_g8(2, eng, max_len=400), lambda a, b: E7._same_weights(b, a), 18.0, 2.0 ** -7),
    "gqa": (lambda eng: EG._decoder(2, eng, max_len=1100), lambda a, b: EG._same_weights(a, b), 20.0, 2.0 ** -6),
}
CASES = [(f, p) for f, ps in (("7b", (126, 127, 128, 300, 1021)), ("g8", (127, 300)), ("gqa", (126, 127, 128, 300, 1021)))
         for p in ps]
MAGNITUDES = (16.0, 64.0, 256.0, 1024.0, 4096.0)


@functools.lru_cache(maxsize=None)
def _pair(family):
    """the launch and the stage-wise step on the same weights; built once, every test plants its own history"""
    make, same, _, _ = FAMILIES[family]
    a, b = make(True), make(False)
    same(a, b)
    assert a.block_eng and not b.block_eng
    return a, b


def _positions(pos0):
    if pos0 <= 300:
        return list(range(pos0))
    ts = sorted(set(range(0, pos0, 17)) | {1, 2, 3, pos0 - 1})
    assert len(ts) >= 64 and {t % 8 for t in ts} == set(range(8)) and {t % 16 for t in ts} == set(range(16))
    return ts


def _plantings(dec, pos0):
    """-> a list of (block, KV head, position) index tensors: in each planting every (block, KV head) has one row, and
    over the list every position of _positions(pos0) is some head's row (the last planting wraps around)"""
    layers, kvh = dec.kcache.shape[0], dec.kcache.shape[1]
    slots = [(l, g) for l in range(layers) for g in range(kvh)]
    ts = _positions(pos0)
    out = []
    for n in range(0, len(ts), len(slots)):
        rows = [ts[(n + i) % len(ts)] for i in range(len(slots))]
        out.append((torch.tensor([s[0] for s in slots], device=DEV), torch.tensor([s[1] for s in slots], device=DEV),
                    torch.tensor(rows, device=DEV)))
    return out


def _signs(dec):
    g = torch.Generator().manual_seed(5)
    n = dec.kcache.shape[0] * dec.kcache.shape[1]
    return (torch.randint(0, 2, (n, dec.kcache.shape[3]), generator=g) * 2 - 1).to(torch.float16).to(DEV)


def _plant(dec, pos0, planting, magnitude, without=None):
    """the counted-keys history: all of both caches zero, one row of +-magnitude per (block, KV head) -- but for slot
    `without`, whose row stays zero"""
    dec.reset(first_token=7)
    L, G, T = planting
    rows = _signs(dec) * magnitude
    if without is not None:
        rows[without] = 0
    with torch.no_grad():
        dec.kcache.zero_()
        dec.vcache.zero_()
        dec.vcache[L, G, T] = rows
        dec.pos.fill_(pos0)


def _ulps_dev(la, lb):
    """max |la - lb| in fp16 ulps of rms(lb), on the device"""
    rms = lb.pow(2).mean().sqrt()
    return (la - lb).abs().max() / torch.exp2(torch.floor(torch.log2(rms)) - 10)


def _new_rows(a, b, p, block=0):
    """the largest difference of block 0's new rows relative to their maximum, K and V, on the device"""
    d = [(ca[block, :, p].float() - cb[block, :, p].float()).abs().max() / cb[block, :, p].float().abs().max()
         for ca, cb in ((a.kcache, b.kcache), (a.vcache, b.vcache))]
    return torch.stack(d).max()


def _teeth(b, pos0, planting, bound):
    """on the stage-wise decoder alone: the smallest magnitude at which a single head's missing row moves the logits by
    >= 10 bounds, in the first block and in the last -> (magnitude, the movements)"""
    slots = planting[0].numel()
    for magnitude in MAGNITUDES:
        with torch.no_grad():
            _plant(b, pos0, planting, magnitude)
            full = b.step().float().clone()
            moves = []
            for without in (0, slots - 1):
                _plant(b, pos0, planting, magnitude, without)
                moves.append(_ulps_dev(b.step().float(), full))
        moves = torch.stack(moves).tolist()
        if min(moves) >= 10 * bound:
            return magnitude, moves
    raise AssertionError(f"a missing row moves the logits by {moves} ulps at magnitude {magnitude}: below 10 x {bound}")


@pytest.mark.parametrize("family,pos0", CASES)
def test_counted_keys(family, pos0):
    """Observed on an MI355X (profiles/attn_hard_cases.txt), launch against stage-wise in fp16 ulps of rms(logits): 7B launch
    8.00 at 126 / 127 / 128, 4.00 at 300 and 1021 (bound 16); G8 8.00 at 127 and 300 (bound 18); 8192-wide 6.94, 6.00, 6.00, 6.00,
    8.00 at 126 .. 1021 (bound 20).  Magnitude 16 (G8), 64, and 256 at 1021; a missing row moves the logits by 185 .. 1234 ulps.
    Block 0's new rows differ by <= 5.9e-4 of their maximum."""
    a, b = _pair(family)
    _, _, bound, row_bound = FAMILIES[family]
    plantings = _plantings(a, pos0)
    magnitude, moves = _teeth(b, pos0, plantings[0], bound)
    errs, rows = [], []
    with torch.no_grad():
        for planting in plantings:
            for dec in (a, b):
                _plant(dec, pos0, planting, magnitude)
            la, lb = a.step().float().clone(), b.step().float().clone()
            errs.append(_ulps_dev(la, lb))
            rows.append(_new_rows(a, b, pos0))
    assert a.engine_status() == 0
    errs, rows = torch.stack(errs).tolist(), torch.stack(rows).tolist()
    print(f"{family} counted keys at {pos0}: magnitude {magnitude:g}, a missing row moves the logits by {min(moves):.0f} ulps; "
          f"{len(plantings)} plantings, launch against stage-wise <= {max(errs):.2f} ulps of rms(logits) (bound {bound:g}), "
          f"block 0's new rows <= {max(rows):.2e} (bound {row_bound:.2e})")
    assert all(e <= bound for e in errs), (max(errs), bound)           # (NaN fails too)
    assert all(r <= row_bound for r in rows), (max(rows), row_bound)


@pytest.mark.parametrize("family,pos0", CASES)
def test_sharp_history(family, pos0):
    """K cache = 4 * randn, V cache = 0.5 * randn below pos0, three steps, tokens kept equal.
    Observed on an MI355X (profiles/attn_hard_cases.txt), the largest of the three steps in fp16 ulps of rms(logits): 7B launch
    5.50, 12.00, 10.00, 6.25, 10.00 at 126 .. 1021 (bound 16); G8 5.12, 10.00 (bound 18); 8192-wide 10.00, 9.25, 11.50, 10.00,
    11.00 (bound 20) -- inside the bounds of the flat histories, which therefore stay as they are."""
    a, b = _pair(family)
    _, _, bound, row_bound = FAMILIES[family]
    g = torch.Generator(device=DEV).manual_seed(pos0)
    errs, rows = [], []
    with torch.no_grad():
        kc = (torch.randn(a.kcache[..., :pos0, :].shape, generator=g, device=DEV) * 4.0).half()
        vc = (torch.randn(a.vcache[..., :pos0, :].shape, generator=g, device=DEV) * 0.5).half()
        for dec in (a, b):
            dec.reset(first_token=7)
            dec.kcache.zero_()
            dec.vcache.zero_()
            dec.kcache[..., :pos0, :].copy_(kc)
            dec.vcache[..., :pos0, :].copy_(vc)
            dec.pos.fill_(pos0)
        for t in range(3):
            la, lb = a.step().float().clone(), b.step().float().clone()
            errs.append(_ulps_dev(la, lb))
            rows.append(_new_rows(a, b, pos0 + t))
            a.tok.copy_(b.tok)
    assert a.engine_status() == 0
    errs, rows = torch.stack(errs).tolist(), torch.stack(rows).tolist()
    print(f"{family} sharp history at {pos0}: launch against stage-wise {', '.join(f'{e:.2f}' for e in errs)} ulps of rms(logits) "
          f"(bound {bound:g}), block 0's new rows <= {max(rows):.2e} (bound {row_bound:.2e})")
    assert all(e <= bound for e in errs), (errs, bound)
    assert all(r <= row_bound for r in rows), (rows, row_bound)
    assert torch.equal(a.kcache[..., :pos0, :], kc) and torch.equal(a.vcache[..., :pos0, :], vc)
