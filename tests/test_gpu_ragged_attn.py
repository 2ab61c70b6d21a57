"""quip_lib::rope_attn_ragged on the device (csrc/ragged_attn.hip.h).  The oracle is the launch's own invariant: segment s's
out rows and cache rows are BIT identical to quip_lib::rope_attn_chunk (tests/test_gpu_chunk_attn.py holds that one to
float64 attention) run on that segment alone against that slot's cache slice -- whatever the other segments are and in
whatever order they come.  So everything here is torch.equal; the one tolerance is the existing bound between the chunk
and the decode launch (2 * BOUND_U of tests/test_chunk_attn_host.py) for a one-row segment."""
import functools

import pytest
import torch

from tests.test_chunk_attn_host import BOUND_U, MAX_LEN, SHAPES, WINDOWS, first_key

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 777.0
BATCH = 5
# boundaries inside a 64-row tile, a 1-row segment at position 0, a segment that is exactly one tile; slot 1 is not named
SLOTS, ROWS, POSITIONS = (2, 0, 3, 4), (70, 1, 33, 64), (130, 0, 61, 300)
IDLE, IDLE_POS = 1, 17
CASES = [(s, w) for s in SHAPES for w in WINDOWS]


def _ops():
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.chunk_attn  # noqa: F401
    import quip_for_all_amd.ragged_attn  # noqa: F401
    return torch.ops.quip_lib


@functools.lru_cache(maxsize=None)
def _tables(hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(MAX_LEN, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


def _pos_tensor(positions=POSITIONS, slots=SLOTS):
    pos = [IDLE_POS] * BATCH
    for b, p in zip(slots, positions):
        pos[b] = p
    return torch.tensor(pos, dtype=torch.long, device=DEV)


def _offsets(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + r)
    return off


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """randn q / k / v per segment (a tuple, in the order of SLOTS), a B = 5 cache with randn rows below each slot's
    position and canaries from it on (read only: every launch gets clones)"""
    heads, kvh, hd = shape
    g = torch.Generator().manual_seed(7 + hd + 10 * heads + kvh)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.float16).to(DEV)  # noqa: E731
    q, k, v = (tuple(r(n, h, hd) for n in ROWS) for h in (heads, kvh, kvh))
    kc, vc = r(BATCH, kvh, MAX_LEN, hd), r(BATCH, kvh, MAX_LEN, hd)
    for b, p in enumerate(_pos_tensor().tolist()):
        kc[b, :, p:], vc[b, :, p:] = CANARY, CANARY
    return q, k, v, kc, vc


def _ragged(shape, window, q, k, v, kc, vc, pos, order=range(len(SLOTS))):
    """one ragged launch on the segments in `order` -> the out rows per segment, indexed as SLOTS is"""
    cos, sin = _tables(shape[2])
    order = list(order)
    out = _ops().rope_attn_ragged(torch.cat([q[j] for j in order]), torch.cat([k[j] for j in order]),
                                  torch.cat([v[j] for j in order]), cos, sin, pos, [SLOTS[j] for j in order],
                                  [ROWS[j] for j in order], kc, vc, window)
    off = _offsets([ROWS[j] for j in order])
    res = [None] * len(SLOTS)
    for n, j in enumerate(order):
        res[j] = out[off[n]:off[n + 1]]
    return res


@functools.lru_cache(maxsize=None)
def _case(shape, window):
    """computed once, shared, read only: the ragged launch on all segments, and rope_attn_chunk on every segment alone
    against its slot's slice of the same initial cache"""
    q, k, v, kc0, vc0 = _inputs(shape)
    cos, sin = _tables(shape[2])
    kc, vc = kc0.clone(), vc0.clone()
    out = _ragged(shape, window, q, k, v, kc, vc, _pos_tensor())
    ref_out, ref_kc, ref_vc = [], [], []
    for j, (b, p) in enumerate(zip(SLOTS, POSITIONS)):
        kcb, vcb = kc0[b].clone(), vc0[b].clone()
        ref_out.append(_ops().rope_attn_chunk(q[j], k[j], v[j], cos, sin, torch.tensor([p], dtype=torch.long, device=DEV),
                                              kcb, vcb, window))
        ref_kc.append(kcb)
        ref_vc.append(vcb)
    torch.cuda.synchronize()
    return dict(out=out, kc=kc, vc=vc, ref_out=ref_out, ref_kc=ref_kc, ref_vc=ref_vc)


@pytest.mark.parametrize("shape,window", CASES)
def test_segments_equal_single_chunk_launches(shape, window):
    q, k, v, kc0, vc0 = _inputs(shape)
    c = _case(shape, window)
    for j, (b, n, p) in enumerate(zip(SLOTS, ROWS, POSITIONS)):
        assert torch.isfinite(c["ref_out"][j]).all()
        assert torch.equal(c["out"][j], c["ref_out"][j]), (j, b)
        assert torch.equal(c["kc"][b], c["ref_kc"][j]) and torch.equal(c["vc"][b], c["ref_vc"][j]), (j, b)
        # appended rows, nothing below and no canary behind them
        assert torch.equal(c["vc"][b][:, p:p + n], v[j].transpose(0, 1))
        assert torch.equal(c["kc"][b][:, :p], kc0[b][:, :p]) and torch.equal(c["vc"][b][:, :p], vc0[b][:, :p])
        assert bool((c["kc"][b][:, p + n:] == CANARY).all()) and bool((c["vc"][b][:, p + n:] == CANARY).all())
    assert torch.equal(c["kc"][IDLE], kc0[IDLE]) and torch.equal(c["vc"][IDLE], vc0[IDLE])


@pytest.mark.parametrize("shape,window", CASES)
@pytest.mark.parametrize("order", [(3, 1, 0, 2), (1, 2, 3, 0)])
def test_order_independence(shape, window, order):
    q, k, v, kc0, vc0 = _inputs(shape)
    c = _case(shape, window)
    kc, vc = kc0.clone(), vc0.clone()
    out = _ragged(shape, window, q, k, v, kc, vc, _pos_tensor(), order)
    assert all(torch.equal(out[j], c["out"][j]) for j in range(len(SLOTS)))
    assert torch.equal(kc, c["kc"]) and torch.equal(vc, c["vc"])


@pytest.mark.parametrize("shape,window", CASES)
@pytest.mark.parametrize("j", range(len(SLOTS)))
def test_one_segment(shape, window, j):
    """a single segment is rope_attn_chunk; at one row it stays inside the chunk launch's bound against rope_attn_decode"""
    heads, kvh, hd = shape
    q, k, v, kc0, vc0 = _inputs(shape)
    c = _case(shape, window)
    b, n, p = SLOTS[j], ROWS[j], POSITIONS[j]
    cos, sin = _tables(hd)
    kc, vc = kc0.clone(), vc0.clone()
    out = _ops().rope_attn_ragged(q[j], k[j], v[j], cos, sin, _pos_tensor(), [b], [n], kc, vc, window)
    assert torch.equal(out, c["ref_out"][j])
    assert torch.equal(kc[b], c["ref_kc"][j]) and torch.equal(vc[b], c["ref_vc"][j])
    for o in range(BATCH):
        if o != b:
            assert torch.equal(kc[o], kc0[o]) and torch.equal(vc[o], vc0[o])
    # one row (the last of the segment, behind the rows the launch above appended) against the decode launch
    last = p + n - 1
    pos = _pos_tensor()
    pos[b] = last
    kc1, vc1 = kc.clone(), vc.clone()
    got = _ops().rope_attn_ragged(q[j][-1:], k[j][-1:], v[j][-1:], cos, sin, pos, [b], [1], kc1, vc1, window)
    assert torch.equal(got[0], c["ref_out"][j][-1])            # rule (2): any split of a chunk gives the same bits
    kcd, vcd = kc[b].clone(), vc[b].clone()
    dec = _ops().rope_attn_decode(q[j][-1], k[j][-1], v[j][-1], cos, sin, pos[b:b + 1], kcd, vcd, None, window)
    assert torch.equal(kc1[b], kcd) and torch.equal(vc1[b], vcd)
    a = first_key(last, window)
    u = vcd.float().abs()[:, a:last + 1].amax(dim=(1, 2)).repeat_interleave(heads // kvh) * 2.0 ** -11      # per head
    err = float(((got[0].float() - dec.float()).abs().amax(dim=1) / u).max())
    print(f"shape {shape} window {window} segment {j}: ragged vs decode {err:.3f} u (bound {2 * BOUND_U})")
    assert err <= 2 * BOUND_U


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bad", ["-1", "max_len - rows + 1", "10 ** 12"])
def test_range_rule_per_segment(shape, bad):
    j = 2
    positions = list(POSITIONS)
    positions[j] = eval(bad, {"max_len": MAX_LEN, "rows": ROWS[j]})
    q, k, v, kc0, vc0 = _inputs(shape)
    c = _case(shape, 0)
    kc, vc = kc0.clone(), vc0.clone()
    out = _ragged(shape, 0, q, k, v, kc, vc, _pos_tensor(positions))
    assert torch.isnan(out[j]).all()
    assert torch.equal(kc[SLOTS[j]], kc0[SLOTS[j]]) and torch.equal(vc[SLOTS[j]], vc0[SLOTS[j]])
    for o in range(len(SLOTS)):
        if o != j:
            assert torch.equal(out[o], c["out"][o]), o
            assert torch.equal(kc[SLOTS[o]], c["kc"][SLOTS[o]]) and torch.equal(vc[SLOTS[o]], c["vc"][SLOTS[o]]), o
    assert torch.equal(kc[IDLE], kc0[IDLE]) and torch.equal(vc[IDLE], vc0[IDLE])


@pytest.mark.parametrize("shape,window", CASES)
@pytest.mark.parametrize("j", [0, 3])
def test_isolation_without_tolerance(shape, window, j):
    """other rows / another slot's cache never reach a segment: replace them, no bit of the other segments moves"""
    q, k, v, kc0, vc0 = _inputs(shape)
    c = _case(shape, window)
    others = [o for o in range(len(SLOTS)) if o != j]
    q2, k2, v2 = (tuple(torch.randn_like(x) if o == j else x for o, x in enumerate(t)) for t in (q, k, v))
    out = _ragged(shape, window, q2, k2, v2, kc0.clone(), vc0.clone(), _pos_tensor())
    assert all(torch.equal(out[o], c["out"][o]) for o in others)
    assert all(not torch.equal(out[j][:, h], c["out"][j][:, h]) for h in range(shape[0]))
    kc, vc = kc0.clone(), vc0.clone()
    kc[SLOTS[j]], vc[SLOTS[j]] = torch.randn_like(kc[SLOTS[j]]), torch.randn_like(vc[SLOTS[j]])
    out = _ragged(shape, window, q, k, v, kc, vc, _pos_tensor())
    assert all(torch.equal(out[o], c["out"][o]) for o in others)
    assert not torch.equal(out[j], c["out"][j])
    for o in others:
        assert torch.equal(kc[SLOTS[o]], c["kc"][SLOTS[o]]) and torch.equal(vc[SLOTS[o]], c["vc"][SLOTS[o]])


def test_op_registration():
    shape = SHAPES[0]
    q, k, v, kc0, vc0 = _inputs(shape)
    cos, sin = _tables(shape[2])
    torch.library.opcheck(_ops().rope_attn_ragged.default,
                          (torch.cat(q), torch.cat(k), torch.cat(v), cos, sin, _pos_tensor(), list(SLOTS), list(ROWS),
                           kc0.clone(), vc0.clone(), 16), test_utils=("test_schema", "test_faketensor"))


def test_the_op_refuses_duplicate_slots_and_a_wrong_row_sum():
    shape = SHAPES[0]
    q, k, v, kc0, vc0 = _inputs(shape)
    cos, sin = _tables(shape[2])
    args = (torch.cat(q), torch.cat(k), torch.cat(v), cos, sin, _pos_tensor())
    with pytest.raises(ValueError, match="distinct"):
        _ops().rope_attn_ragged(*args, [2, 0, 2, 4], list(ROWS), kc0.clone(), vc0.clone(), 0)
    with pytest.raises(ValueError, match="sum"):
        _ops().rope_attn_ragged(*args, list(SLOTS), [70, 1, 33, 63], kc0.clone(), vc0.clone(), 0)
