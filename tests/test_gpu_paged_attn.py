"""quip_lib::rope_attn_decode_paged and quip_lib::rope_attn_ragged_paged on the device (csrc/paged_attn.hip.h).  Paging
changes where a cache row lives and nothing about what is computed with it, so the oracle is the contiguous launch
(rope_attn_decode_batched, rope_attn_ragged) on the rows gathered through the table, and everything is torch.equal.

The pool is the slice big[1:-1] of an allocation with one guard page in front and one behind, all of it poisoned before
the cached rows are written: an addressing mistake with entry -1 or n_pages lands in owned memory and fails a
comparison.  After every launch the WHOLE allocation is compared with what it must be: its prior bits with the appended
rows replaced by the contiguous launch's."""
import functools
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PAGE, MAX_PAGES, N_PAGES = 64, 6, 20
MAX_LEN = PAGE * MAX_PAGES
POISON = 777.0
SHAPES = ((4, 2, 64), (4, 2, 128), (4, 4, 64), (4, 4, 128))          # heads, kv_heads, head_dim
WINDOWS = (0, 100)
CASES = [(s, w) for s in SHAPES for w in WINDOWS]
# decode, B = 3: the first row of a new page (0, 64, 256), both sides of the split threshold (255, 256), split mode over
# several pages (300, 383)
DECODE_POS = ((0, 64, 256), (1, 65, 300), (63, 127, 383), (255, 383, 1))
# ragged, B = 5: (rows, position) per slot; slot b is segment b
SEGMENTS = ((1, 0), (63, 1), (64, 63), (65, 64), (130, 100))
ORDERS = ((0, 1, 2, 3, 4), (4, 2, 0), (3, 1, 4, 2))


def _ops():
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.batch_decode  # noqa: F401
    import quip_for_all_amd.paged_attn  # noqa: F401
    return torch.ops.quip_lib


@functools.lru_cache(maxsize=None)
def _tables(hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(MAX_LEN, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


def _gen(shape, salt):
    heads, kvh, hd = shape
    g = torch.Generator().manual_seed(salt + hd + 10 * heads + kvh)
    return lambda *s: torch.randn(*s, generator=g).to(torch.float16).to(DEV)


def _assignment(pages_per_slot, seed):
    """a seeded random assignment: pages out of order and interleaved between the slots; -1 behind a slot's pages"""
    ids = list(range(N_PAGES))
    random.Random(seed).shuffle(ids)
    table = [[-1] * MAX_PAGES for _ in pages_per_slot]
    for j in range(MAX_PAGES):                      # page j of every slot before page j + 1 of any: interleaved
        for b, n in enumerate(pages_per_slot):
            if j < n:
                table[b][j] = ids.pop()
    return table


def _pool(contig, table):
    """(big, pool): the poisoned allocation with guards and its slice, holding contig (B, kvh, MAX_LEN, hd) through table"""
    B, kvh, _, hd = contig.shape
    big = torch.full((N_PAGES + 2, kvh, PAGE, hd), POISON, dtype=torch.float16, device=DEV)
    for b, row in enumerate(table):
        for j, p in enumerate(row):
            if 0 <= p < N_PAGES:
                big[1 + p] = contig[b, :, PAGE * j:PAGE * (j + 1)]
    return big, big[1:-1]


def _expected(big0, table, contig_after, spans):
    """big0 with rows [t0, t1) of slot b, for (b, t0, t1) in spans, taken from the contiguous cache after its launch"""
    e = big0.clone()
    for b, t0, t1 in spans:
        for j in range(t0 // PAGE, (t1 - 1) // PAGE + 1):
            lo, hi = max(t0, PAGE * j), min(t1, PAGE * (j + 1))
            e[1 + table[b][j], :, lo - PAGE * j:hi - PAGE * j] = contig_after[b, :, lo:hi]
    return e


def _dev_table(table):
    return torch.tensor(table, dtype=torch.int32, device=DEV)


def _workspace(B, heads, hd):
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    return rope_attn_batched_workspace(B, heads, hd, DEV)


# ---- decode
@functools.lru_cache(maxsize=None)
def _decode_inputs(shape):
    heads, kvh, hd = shape
    r = _gen(shape, 11)
    return r(3, heads, hd), r(3, kvh, hd), r(3, kvh, hd), r(3, kvh, MAX_LEN, hd), r(3, kvh, MAX_LEN, hd)


def _decode_pair(shape, window, positions, table, ws_paged, ws_contig, table_for_launch=None):
    """the paged launch and the contiguous one on the same rows -> everything the tests compare"""
    q, k, v, kc0, vc0 = _decode_inputs(shape)
    cos, sin = _tables(shape[2])
    pos = torch.tensor(positions, dtype=torch.long, device=DEV)
    (bigk, kpool), (bigv, vpool) = _pool(kc0, table), _pool(vc0, table)
    bigk0, bigv0 = bigk.clone(), bigv.clone()
    out = _ops().rope_attn_decode_paged(q, k, v, cos, sin, pos, _dev_table(table_for_launch or table), kpool, vpool, ws_paged,
                                        window)
    kc, vc = kc0.clone(), vc0.clone()
    ref = _ops().rope_attn_decode_batched(q, k, v, cos, sin, pos, kc, vc, ws_contig, window)
    torch.cuda.synchronize()
    return dict(out=out, ref=ref, bigk=bigk, bigv=bigv, bigk0=bigk0, bigv0=bigv0, kc=kc, vc=vc)


@pytest.mark.parametrize("shape,window", CASES)
def test_decode_equals_the_contiguous_launch(shape, window):
    table = _assignment((MAX_PAGES,) * 3, 5)
    heads, kvh, hd = shape
    for use_ws in (False, True):
        # one workspace for all position sets: its reuse across launches has to stay exact
        wp, wc = (_workspace(3, heads, hd), _workspace(3, heads, hd)) if use_ws else (None, None)
        for positions in DECODE_POS:
            c = _decode_pair(shape, window, positions, table, wp, wc)
            assert torch.isfinite(c["ref"]).all()
            assert torch.equal(c["out"], c["ref"]), (positions, use_ws)
            spans = [(b, p, p + 1) for b, p in enumerate(positions)]
            assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans)), (positions, use_ws)
            assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans)), (positions, use_ws)
        if use_ws:
            assert torch.equal(wp, wc) and not bool(wp[-3 * heads * 4:].any())          # the arrival counters are back at zero


@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("bad", (-1, N_PAGES))
def test_decode_refuses_an_invalid_table_entry(shape, bad):
    table = _assignment((MAX_PAGES,) * 3, 6)
    heads, kvh, hd = shape
    positions = (65, 300, 127)
    for use_ws in (False, True):
        for page in (1, 4):                                   # a page slot 1 reads, the page it appends to
            wp, wc = (_workspace(3, heads, hd), _workspace(3, heads, hd)) if use_ws else (None, None)
            broken = [list(r) for r in table]
            broken[1][page] = bad
            c = _decode_pair(shape, 0, positions, table, wp, wc, table_for_launch=broken)
            assert bool(torch.isnan(c["out"][1]).all())
            assert torch.equal(c["out"][0], c["ref"][0]) and torch.equal(c["out"][2], c["ref"][2])
            spans = [(0, 65, 66), (2, 127, 128)]              # nothing of slot 1
            assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans))
            assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans))
            if use_ws:
                # the refused sequence left the workspace alone: a valid launch on the same workspace stays exact
                c = _decode_pair(shape, 0, positions, table, wp, wc)
                assert torch.equal(c["out"], c["ref"])
    # below the window's first page (position 300, window 100: first key 201, page 3) nothing is examined
    broken = [list(r) for r in table]
    broken[1][0] = broken[1][2] = bad
    c = _decode_pair(shape, 100, positions, table, None, None, table_for_launch=broken)
    assert torch.equal(c["out"], c["ref"])
    spans = [(b, p, p + 1) for b, p in enumerate(positions)]
    assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans))
    assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans))


# ---- ragged
@functools.lru_cache(maxsize=None)
def _ragged_inputs(shape):
    heads, kvh, hd = shape
    r = _gen(shape, 23)
    q, k, v = (tuple(r(n, h, hd) for n, _ in SEGMENTS) for h in (heads, kvh, kvh))
    return q, k, v, r(5, kvh, MAX_LEN, hd), r(5, kvh, MAX_LEN, hd)


def _ragged_pair(shape, window, order, table, kc0, vc0, positions, table_for_launch=None, rows=None):
    q, k, v, _, _ = _ragged_inputs(shape)
    rows = rows or [n for n, _ in SEGMENTS]
    cos, sin = _tables(shape[2])
    pos = torch.tensor(positions, dtype=torch.long, device=DEV)
    (bigk, kpool), (bigv, vpool) = _pool(kc0, table), _pool(vc0, table)
    bigk0, bigv0 = bigk.clone(), bigv.clone()
    cat = lambda xs: torch.cat([xs[j][:rows[j]] for j in order])  # noqa: E731
    seg_slot, seg_rows = list(order), [rows[j] for j in order]
    out = _ops().rope_attn_ragged_paged(cat(q), cat(k), cat(v), cos, sin, pos, seg_slot, seg_rows,
                                        _dev_table(table_for_launch or table), kpool, vpool, window)
    kc, vc = kc0.clone(), vc0.clone()
    ref = _ops().rope_attn_ragged(cat(q), cat(k), cat(v), cos, sin, pos, seg_slot, seg_rows, kc, vc, window)
    torch.cuda.synchronize()
    off = [0]
    for n in seg_rows:
        off.append(off[-1] + n)
    seg = {j: slice(off[i], off[i + 1]) for i, j in enumerate(order)}
    return dict(out=out, ref=ref, bigk=bigk, bigv=bigv, bigk0=bigk0, bigv0=bigv0, kc=kc, vc=vc, seg=seg)


@pytest.mark.parametrize("shape,window", CASES)
def test_ragged_equals_the_contiguous_launch(shape, window):
    _, _, _, kc0, vc0 = _ragged_inputs(shape)
    positions = [p for _, p in SEGMENTS]
    table = _assignment([(p + n + PAGE - 1) // PAGE for n, p in SEGMENTS], 7)
    for order in ORDERS:
        c = _ragged_pair(shape, window, order, table, kc0, vc0, positions)
        assert torch.isfinite(c["ref"]).all()
        assert torch.equal(c["out"], c["ref"]), order
        spans = [(j, SEGMENTS[j][1], SEGMENTS[j][1] + SEGMENTS[j][0]) for j in order]
        assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans)), order
        assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans)), order


@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("sharers,prefix_pages", ((2, 1), (3, 2), (3, 1), (2, 2)))
def test_ragged_on_a_shared_prefix(shape, sharers, prefix_pages):
    """slots 0 .. sharers-1 name the SAME first pages and then diverge: one starts a fresh page right behind the prefix,
    the others sit 10 and 64 rows into pages of their own"""
    _, _, _, kc0, vc0 = _ragged_inputs(shape)
    P = PAGE * prefix_pages
    kc0, vc0 = kc0.clone(), vc0.clone()
    for b in range(1, sharers):                         # the contiguous oracle holds the prefix once per slot
        kc0[b, :, :P], vc0[b, :, :P] = kc0[0, :, :P], vc0[0, :, :P]
    extra, rows = (0, 10, 64), [n for n, _ in SEGMENTS]
    positions = [P + extra[b] if b < sharers else 5 for b in range(5)]
    order = list(range(sharers)) + [4]                  # and one slot that shares nothing
    table = _assignment([(positions[b] + rows[b] + PAGE - 1) // PAGE for b in range(5)], 8)
    for b in range(1, sharers):
        table[b][:prefix_pages] = table[0][:prefix_pages]
    for window in WINDOWS:
        c = _ragged_pair(shape, window, order, table, kc0, vc0, positions, rows=rows)
        assert torch.isfinite(c["ref"]).all()
        assert torch.equal(c["out"], c["ref"]), window
        spans = [(j, positions[j], positions[j] + rows[j]) for j in order]
        assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans))
        assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans))
        for p in table[0][:prefix_pages]:               # the shared pages keep their bits
            assert torch.equal(c["bigk"][1 + p], c["bigk0"][1 + p]) and torch.equal(c["bigv"][1 + p], c["bigv0"][1 + p])


@pytest.mark.parametrize("shape", SHAPES[:2])
@pytest.mark.parametrize("bad", (-1, N_PAGES))
def test_ragged_refuses_an_invalid_table_entry(shape, bad):
    _, _, _, kc0, vc0 = _ragged_inputs(shape)
    positions = [p for _, p in SEGMENTS]
    table = _assignment([(p + n + PAGE - 1) // PAGE for n, p in SEGMENTS], 9)
    order = (3, 4, 1)
    for page in (0, 3):                                     # segment 4 (130 rows behind 100): a page it reads, one it appends to
        broken = [list(r) for r in table]
        broken[4][page] = bad
        c = _ragged_pair(shape, 0, order, table, kc0, vc0, positions, table_for_launch=broken)
        assert bool(torch.isnan(c["out"][c["seg"][4]]).all())
        for j in (3, 1):
            assert torch.equal(c["out"][c["seg"][j]], c["ref"][c["seg"][j]])
        spans = [(j, SEGMENTS[j][1], SEGMENTS[j][1] + SEGMENTS[j][0]) for j in (3, 1)]
        assert torch.equal(c["bigk"], _expected(c["bigk0"], table, c["kc"], spans))
        assert torch.equal(c["bigv"], _expected(c["bigv0"], table, c["vc"], spans))
    # window 100 behind position 100: the first key of segment 4's first row is 1, page 0 -- nothing below it; behind
    # position 300 (slot 2 moved there, 64 rows) the first key is 201, page 3: pages 0 .. 2 are not examined
    positions2 = list(positions)
    positions2[2] = 300
    table2 = _assignment([1, 1, 6, 3, 4], 10)
    broken = [list(r) for r in table2]
    broken[2][0] = broken[2][2] = bad
    c = _ragged_pair(shape, 100, (2, 0), table2, kc0, vc0, positions2, table_for_launch=broken)
    assert torch.isfinite(c["ref"]).all() and torch.equal(c["out"], c["ref"])
    spans = [(2, 300, 364), (0, 0, 1)]
    assert torch.equal(c["bigk"], _expected(c["bigk0"], table2, c["kc"], spans))
    assert torch.equal(c["bigv"], _expected(c["bigv0"], table2, c["vc"], spans))


def test_wrappers_refuse_what_they_can_see():
    heads, kvh, hd = SHAPES[0]
    q, k, v, kc0, vc0 = _decode_inputs(SHAPES[0])
    cos, sin = _tables(hd)
    pos = torch.zeros(3, dtype=torch.long, device=DEV)
    table = _dev_table(_assignment((MAX_PAGES,) * 3, 5))
    _, kpool = _pool(kc0, [[-1] * MAX_PAGES] * 3)
    f = _ops().rope_attn_decode_paged
    with pytest.raises(ValueError):
        f(q, k, v, cos, sin, pos, table.long(), kpool, kpool.clone(), None, 0)                     # dtype of the table
    with pytest.raises(ValueError):
        f(q, k, v, cos, sin, pos, table[:, :5], kpool, kpool.clone(), None, 0)                     # not contiguous
    with pytest.raises(ValueError):
        f(q, k, v, cos, sin, pos, table[:, :5].contiguous(), kpool, kpool.clone(), None, 0)        # 320 < 384 rows of cos
    with pytest.raises(ValueError):
        f(q, k, v, cos, sin, pos, table, kpool[:, :, :32].contiguous(), kpool.clone(), None, 0)    # not 64-row pages
    with pytest.raises(ValueError):
        f(q, k, v, cos, sin, pos, table.cpu(), kpool, kpool.clone(), None, 0)                      # device
