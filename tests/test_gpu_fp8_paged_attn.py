"""quip_lib::rope_attn_decode_paged_f8 and quip_lib::rope_attn_ragged_paged_f8 on the device (csrc/paged_attn.hip.h): the
two paged launches on pools of OCP e4m3fn bytes, a byte c meaning e4m3fn(c) * 2^e.

Dequantisation is exact, so the fp16 paged launches are a bit-for-bit oracle wherever the appended rows are
representable (test 1: quarter-turn rotary tables, representable k / v); the bytes a launch appends are the CPU oracle
paged_attn.quant_f8 of the rows the fp16 launch appends (test 2); the rows a launch appends are used by it as stored --
the round-trip rule -- so a chunk split into consecutive launches gives the same bits (test 3) and the decode output is
an attention over the pool as it is AFTER the launch (test 4); an invalid table entry is refused as by the fp16 launches
(test 5).

The harness is that of test_gpu_paged_attn.py: the pool is the slice big[1:-1] of a poisoned allocation with a guard page
on either side, the table is shuffled, and after every launch the WHOLE allocation is compared with what it must be."""
import functools

import pytest
import torch

from tests.test_gpu_paged_attn import (DECODE_POS, MAX_LEN, MAX_PAGES, N_PAGES, ORDERS, PAGE, SEGMENTS, _assignment,
                                       _dev_table, _ops, _tables, _workspace)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POISON = 0x7E                                              # 448 * 2^e: a finite fp16 value at every exponent
SHAPES = ((4, 2, 64), (4, 2, 128))                         # heads, kv_heads, head_dim
WINDOWS = (0, 100)
EXPS = ((0, 0), (-8, -8), (-3, 2))                         # (k_exp, v_exp)
CASES = [(s, w, e) for s in SHAPES for w in WINDOWS for e in EXPS]


def _F():
    from quip_for_all_amd import paged_attn
    return paged_attn


@functools.lru_cache(maxsize=None)
def _lut(e):
    """dequantisation as a table on the device: byte -> fp16 (NaN codes -> NaN)"""
    return _F().dequant_f8(torch.arange(256, dtype=torch.uint8), e).to(DEV)


def _deq(b, e):
    return _lut(e)[b.long()]


def _quant(x, e):
    """the CPU oracle, result back on the device"""
    return _F().quant_f8(x.cpu(), e).to(DEV)


def _bits(x):
    return x.view(torch.int16)


@functools.lru_cache(maxsize=None)
def _quarter_tables(hd):
    """cos / sin of exact quarter turns: entries in {1, 0, -1}, angle index (t (i + 1)) mod 4 for frequency i"""
    t = torch.arange(MAX_LEN)[:, None]
    i = torch.arange(hd // 2)[None, :]
    a = (t * (i + 1)) % 4
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[a]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[a]
    return torch.cat([cos, cos], -1).contiguous().to(DEV), torch.cat([sin, sin], -1).contiguous().to(DEV)


class _rand:
    """seeded CPU draws"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)

    def __call__(self, *s):
        return torch.randn(*s, generator=self.g)

    def uniform(self, *s):
        return torch.rand(*s, generator=self.g)


def _cached_bytes(r, e, *shape):
    """cache contents: at exponent -8 uniform over all 254 non-NaN codes (values <= 1.75: every code passes through the
    kernels, the outputs stay finite), else quant(randn)"""
    if e == -8:
        codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)
        return codes[(r.uniform(*shape) * 254).long().clamp(max=253)].to(DEV)
    return _F().quant_f8(r(*shape), e).to(DEV)


def _representable(r, e, *shape):
    """fp16 inputs that are e4m3fn values at exponent e already, none of them zero"""
    b = _F().quant_f8(r(*shape), e)
    b = torch.where(b & 0x7f == 0, b | 0x38, b)
    return _F().dequant_f8(b, e).to(DEV)


def _pool8(contig, table):
    """(big, pool): the poisoned uint8 allocation with guards and its slice, holding contig (B, kvh, MAX_LEN, hd)"""
    B, kvh, _, hd = contig.shape
    big = torch.full((N_PAGES + 2, kvh, PAGE, hd), POISON, dtype=torch.uint8, device=DEV)
    for b, row in enumerate(table):
        for j, p in enumerate(row):
            if 0 <= p < N_PAGES:
                big[1 + p] = contig[b, :, PAGE * j:PAGE * (j + 1)]
    return big, big[1:-1]


def _mask(big, table, spans):
    """True at rows [t0, t1) of slot b, for (b, t0, t1) in spans, of the allocation"""
    m = torch.zeros(big.shape, dtype=torch.bool, device=DEV)
    for b, t0, t1 in spans:
        for t in range(t0, t1):
            m[1 + table[b][t // PAGE], :, t % PAGE] = True
    return m


def _check_pools(c, table, spans, exps, what):
    """the fp8 allocations against the fp16 ones after the twin launches: outside the appended rows nothing moved (guards
    included); the appended bytes are the CPU oracle of the fp16 launch's rows, NaN compared by the mask"""
    for big8, big8_0, big16, e in ((c["bigk8"], c["bigk8_0"], c["bigk16"], exps[0]), (c["bigv8"], c["bigv8_0"], c["bigv16"], exps[1])):
        m = _mask(big8, table, spans)
        want = torch.where(m, _quant(big16, e), big8_0)
        nan = want & 0x7f == 0x7f
        assert torch.equal(big8 & 0x7f == 0x7f, nan), what
        assert torch.equal(torch.where(nan, want, big8), want), what


def _twin_decode(shape, window, exps, positions, table, q, k, v, kc8, vc8, cos, sin, ws8=None, ws16=None, table_for_launch=None):
    """the fp8 launch, and the fp16 paged launch on pools holding the dequantised bytes"""
    pos = torch.tensor(positions, dtype=torch.long, device=DEV)
    (bigk8, kp8), (bigv8, vp8) = _pool8(kc8, table), _pool8(vc8, table)
    bigk8_0, bigv8_0 = bigk8.clone(), bigv8.clone()
    bigk16, bigv16 = _deq(bigk8, exps[0]), _deq(bigv8, exps[1])
    t8 = _dev_table(table_for_launch or table)
    out = _ops().rope_attn_decode_paged_f8(q, k, v, cos, sin, pos, t8, kp8, vp8, ws8, window, exps[0], exps[1])
    ref = _ops().rope_attn_decode_paged(q, k, v, cos, sin, pos, _dev_table(table), bigk16[1:-1], bigv16[1:-1], ws16, window)
    torch.cuda.synchronize()
    return dict(out=out, ref=ref, bigk8=bigk8, bigv8=bigv8, bigk8_0=bigk8_0, bigv8_0=bigv8_0, bigk16=bigk16, bigv16=bigv16)


def _twin_ragged(window, exps, order, rows, positions, table, q, k, v, kc8, vc8, cos, sin, table_for_launch=None):
    pos = torch.tensor(positions, dtype=torch.long, device=DEV)
    (bigk8, kp8), (bigv8, vp8) = _pool8(kc8, table), _pool8(vc8, table)
    bigk8_0, bigv8_0 = bigk8.clone(), bigv8.clone()
    bigk16, bigv16 = _deq(bigk8, exps[0]), _deq(bigv8, exps[1])
    cat = lambda xs: torch.cat([xs[j][:rows[j]] for j in order])  # noqa: E731
    seg_slot, seg_rows = list(order), [rows[j] for j in order]
    out = _ops().rope_attn_ragged_paged_f8(cat(q), cat(k), cat(v), cos, sin, pos, seg_slot, seg_rows,
                                           _dev_table(table_for_launch or table), kp8, vp8, window, exps[0], exps[1])
    ref = _ops().rope_attn_ragged_paged(cat(q), cat(k), cat(v), cos, sin, pos, seg_slot, seg_rows, _dev_table(table),
                                        bigk16[1:-1], bigv16[1:-1], window)
    torch.cuda.synchronize()
    off = [0]
    for n in seg_rows:
        off.append(off[-1] + n)
    seg = {j: slice(off[i], off[i + 1]) for i, j in enumerate(order)}
    return dict(out=out, ref=ref, bigk8=bigk8, bigv8=bigv8, bigk8_0=bigk8_0, bigv8_0=bigv8_0, bigk16=bigk16, bigv16=bigv16,
                seg=seg)


# ---- inputs (one set per shape and exponent pair, shared by the tests and never modified)
@functools.lru_cache(maxsize=None)
def _decode_inputs(shape, exps, exact):
    heads, kvh, hd = shape
    r = _rand(31 + hd + 7 * exps[0] + exps[1] + 1000 * exact)
    q = r(3, heads, hd).to(torch.float16).to(DEV)
    if exact:
        k, v = _representable(r, exps[0], 3, kvh, hd), _representable(r, exps[1], 3, kvh, hd)
    else:
        k, v = r(3, kvh, hd).to(torch.float16).to(DEV), r(3, kvh, hd).to(torch.float16).to(DEV)
    return q, k, v, _cached_bytes(r, exps[0], 3, kvh, MAX_LEN, hd), _cached_bytes(r, exps[1], 3, kvh, MAX_LEN, hd)


@functools.lru_cache(maxsize=None)
def _ragged_inputs(shape, exps, exact):
    heads, kvh, hd = shape
    r = _rand(57 + hd + 7 * exps[0] + exps[1] + 1000 * exact)
    q = tuple(r(n, heads, hd).to(torch.float16).to(DEV) for n, _ in SEGMENTS)
    if exact:
        k, v = (tuple(_representable(r, e, n, kvh, hd) for n, _ in SEGMENTS) for e in exps)
    else:
        k, v = (tuple(r(n, kvh, hd).to(torch.float16).to(DEV) for n, _ in SEGMENTS) for _ in exps)
    return q, k, v, _cached_bytes(r, exps[0], 5, kvh, MAX_LEN, hd), _cached_bytes(r, exps[1], 5, kvh, MAX_LEN, hd)


def _salt(x, e):
    """rows with what the rounding has to get right in their first dims: saturation (1e4, +-inf), NaN, ties (17 -> 16,
    19 -> 20, -432 -> -448), the subnormal range (half a step ties to zero, below it, 1.5 and 2.5 steps tie to 2)"""
    s, u = 2.0 ** e, 2.0 ** (e - 9)
    salt = torch.tensor([1e4, float("inf"), -float("inf"), float("nan"), 17 * s, 19 * s, -432 * s, 0.5 * u, 0.4 * u, 1.5 * u,
                         -2.5 * u, -1e4], dtype=torch.float32).to(torch.float16).to(DEV)
    x = x.clone()
    x[..., :salt.numel()] = salt
    return x


# ---- 1. exact against the fp16 paged launch
@pytest.mark.parametrize("shape,window,exps", CASES)
def test_decode_gives_the_bits_of_the_fp16_paged_launch(shape, window, exps):
    heads, kvh, hd = shape
    q, k, v, kc8, vc8 = _decode_inputs(shape, exps, True)
    cos, sin = _quarter_tables(hd)
    table = _assignment((MAX_PAGES,) * 3, 5)
    for use_ws in (False, True):
        w8, w16 = (_workspace(3, heads, hd), _workspace(3, heads, hd)) if use_ws else (None, None)
        for positions in DECODE_POS:
            c = _twin_decode(shape, window, exps, positions, table, q, k, v, kc8, vc8, cos, sin, w8, w16)
            assert torch.isfinite(c["ref"]).all()
            assert torch.equal(_bits(c["out"]), _bits(c["ref"])), (positions, use_ws)
            # the pools, dequantised, are the fp16 pools bit for bit; and byte for byte what they must be
            assert torch.equal(_bits(_deq(c["bigk8"], exps[0])), _bits(c["bigk16"])), (positions, use_ws)
            assert torch.equal(_bits(_deq(c["bigv8"], exps[1])), _bits(c["bigv16"])), (positions, use_ws)
            _check_pools(c, table, [(b, p, p + 1) for b, p in enumerate(positions)], exps, (positions, use_ws))
        if use_ws:
            assert torch.equal(w8, w16) and not bool(w8[-3 * heads * 4:].any())          # the arrival counters are back at zero


@pytest.mark.parametrize("shape,window,exps", CASES)
def test_ragged_gives_the_bits_of_the_fp16_paged_launch(shape, window, exps):
    q, k, v, kc8, vc8 = _ragged_inputs(shape, exps, True)
    cos, sin = _quarter_tables(shape[2])
    rows, positions = [n for n, _ in SEGMENTS], [p for _, p in SEGMENTS]
    table = _assignment([(p + n + PAGE - 1) // PAGE for n, p in SEGMENTS], 7)
    for order in ORDERS:
        c = _twin_ragged(window, exps, order, rows, positions, table, q, k, v, kc8, vc8, cos, sin)
        assert torch.isfinite(c["ref"]).all()
        assert torch.equal(_bits(c["out"]), _bits(c["ref"])), order
        assert torch.equal(_bits(_deq(c["bigk8"], exps[0])), _bits(c["bigk16"])), order
        assert torch.equal(_bits(_deq(c["bigv8"], exps[1])), _bits(c["bigv16"])), order
        _check_pools(c, table, [(j, positions[j], positions[j] + rows[j]) for j in order], exps, order)


# ---- 2. rounding on append
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("exps", EXPS)
def test_appended_bytes_are_the_cpu_oracle_of_the_fp16_rows(shape, exps):
    heads, kvh, hd = shape
    cos, sin = _tables(hd)
    q, k, v, kc8, vc8 = _decode_inputs(shape, exps, False)
    k, v = _salt(k, exps[0]), _salt(v, exps[1])
    table = _assignment((MAX_PAGES,) * 3, 5)
    for positions in ((0, 64, 256), (63, 127, 383)):         # position 0: the rotation is the identity, K meets the ties too
        c = _twin_decode(shape, 0, exps, positions, table, q, k, v, kc8, vc8, cos, sin)
        _check_pools(c, table, [(b, p, p + 1) for b, p in enumerate(positions)], exps, positions)
    q, k, v, kc8, vc8 = _ragged_inputs(shape, exps, False)
    k, v = tuple(_salt(x, exps[0]) for x in k), tuple(_salt(x, exps[1]) for x in v)
    rows, positions = [n for n, _ in SEGMENTS], [p for _, p in SEGMENTS]
    table = _assignment([(p + n + PAGE - 1) // PAGE for n, p in SEGMENTS], 7)
    c = _twin_ragged(0, exps, ORDERS[0], rows, positions, table, q, k, v, kc8, vc8, cos, sin)
    _check_pools(c, table, [(j, positions[j], positions[j] + rows[j]) for j in ORDERS[0]], exps, "ragged")
    # the salt arrived: saturated, NaN and zero bytes among the appended V rows (V is not rotated)
    got = c["bigv8"][_mask(c["bigv8"], table, [(0, 0, 1)])].view(kvh, hd)[:, :12].tolist()
    assert all(r[:3] == [0x7e, 0x7e, 0xfe] and r[3] & 0x7f == 0x7f and r[4:] == [0x58, 0x5a, 0xfe, 0, 0, 2, 0x82, 0xfe]
               for r in got), got


# ---- 3. the round-trip rule, ragged: a chunk in one launch or in several
@pytest.mark.parametrize("shape,window,exps", CASES)
def test_a_split_chunk_gives_the_same_bits(shape, window, exps):
    heads, kvh, hd = shape
    cos, sin = _tables(hd)
    q, k, v, kc8, vc8 = _ragged_inputs(shape, exps, False)
    q, k, v = q[4], k[4], v[4]                                 # 130 rows behind position 100, slot 4
    table = _assignment([1, 1, 1, 1, 4], 11)
    results = []
    for split in ((130,), (70, 60), (1, 64, 65)):
        (bigk, kp), (bigv, vp) = _pool8(kc8, table), _pool8(vc8, table)
        bigk[_mask(bigk, table, [(4, 100, 256)])] = POISON      # nothing behind the cached rows yet
        bigv[_mask(bigv, table, [(4, 100, 256)])] = POISON
        outs, r0 = [], 0
        for n in split:
            pos = torch.tensor([0, 0, 0, 0, 100 + r0], dtype=torch.long, device=DEV)
            outs.append(_ops().rope_attn_ragged_paged_f8(q[r0:r0 + n], k[r0:r0 + n], v[r0:r0 + n], cos, sin, pos, [4], [n],
                                                         _dev_table(table), kp, vp, window, exps[0], exps[1]))
            r0 += n
        torch.cuda.synchronize()
        results.append((torch.cat(outs), bigk, bigv))
    out, bigk, bigv = results[0]
    assert torch.isfinite(out).all()
    for o2, k2, v2 in results[1:]:
        assert torch.equal(_bits(out), _bits(o2)) and torch.equal(bigk, k2) and torch.equal(bigv, v2)


# ---- 4. the round-trip rule, decode: the output is an attention over the pool as it is after the launch
def _rotate(x, cos_row, sin_row):
    """rope8 in torch: every operation rounded on its own in fp32, the result to fp16"""
    hd = x.shape[-1]
    xf = x.float()
    rot = torch.cat([-xf[..., hd // 2:], xf[..., :hd // 2]], -1)
    return (xf * cos_row + rot * sin_row).to(torch.float16)


def _attention64(q, positions, window, table, kpool16, vpool16, cos, sin):
    """float64 attention of the rotated q over rows [first, pos] of the (dequantised) pools -> (B, heads, hd)"""
    B, heads, hd = q.shape
    kvh = kpool16.shape[1]
    out = torch.zeros(B, heads, hd, dtype=torch.float64, device=DEV)
    for b, p in enumerate(positions):
        first = max(0, p + 1 - window) if window > 0 else 0
        rows = torch.tensor([(table[b][t // PAGE], t % PAGE) for t in range(first, p + 1)], device=DEV)
        K = kpool16[rows[:, 0], :, rows[:, 1]].double()       # (T, kvh, hd)
        V = vpool16[rows[:, 0], :, rows[:, 1]].double()
        qr = _rotate(q[b], cos[p], sin[p]).double() / hd ** 0.5
        for h in range(heads):
            g = h // (heads // kvh)
            w = torch.softmax(K[:, g] @ qr[h], 0)
            out[b, h] = w @ V[:, g]
    return out


@pytest.mark.parametrize("shape,window,exps", CASES)
def test_decode_scores_the_new_row_as_stored(shape, window, exps):
    """The tolerance is that of an fp16 output: the fp16 paged launch against the same float64 computation on its own
    pool, measured here; the fp8 launch may have twice that launch's maximum error (both launches do the same fp32
    arithmetic on exactly known fp16 values and round the output once, so their errors are of one size; a kernel that
    scored the un-rounded key would be off by the rounding of a key, orders of magnitude more).
    Measured on the MI355X: see profiles/fp8_kv_bench.txt."""
    heads, kvh, hd = shape
    cos, sin = _tables(hd)
    q, k, v, kc8, vc8 = _decode_inputs(shape, exps, False)
    table = _assignment((MAX_PAGES,) * 3, 5)
    err8 = err16 = 0.0
    for use_ws in (False, True):
        w8, w16 = (_workspace(3, heads, hd), _workspace(3, heads, hd)) if use_ws else (None, None)
        for positions in DECODE_POS:
            c = _twin_decode(shape, window, exps, positions, table, q, k, v, kc8, vc8, cos, sin, w8, w16)
            want8 = _attention64(q, positions, window, table, _deq(c["bigk8"], exps[0])[1:-1], _deq(c["bigv8"], exps[1])[1:-1],
                                 cos, sin)
            want16 = _attention64(q, positions, window, table, c["bigk16"][1:-1], c["bigv16"][1:-1], cos, sin)
            assert torch.isfinite(c["out"]).all() and torch.isfinite(c["ref"]).all()
            err8 = max(err8, float((c["out"].double() - want8).abs().max()))
            err16 = max(err16, float((c["ref"].double() - want16).abs().max()))
    line = f"decode vs float64 on the pool after the launch, {shape} window {window} exps {exps}: fp8 {err8:.3e} fp16 {err16:.3e}"
    print(line)
    assert err8 <= 2 * err16, line


# ---- 5. refusals
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bad", (-1, N_PAGES))
def test_an_invalid_table_entry_is_refused(shape, bad):
    heads, kvh, hd = shape
    exps = (-3, 2)
    cos, sin = _quarter_tables(hd)
    q, k, v, kc8, vc8 = _decode_inputs(shape, exps, True)
    table = _assignment((MAX_PAGES,) * 3, 6)
    positions = (65, 300, 127)
    for use_ws in (False, True):
        for page in (1, 4):                                   # a page slot 1 reads, the page it appends to
            w8, w16 = (_workspace(3, heads, hd), _workspace(3, heads, hd)) if use_ws else (None, None)
            broken = [list(r) for r in table]
            broken[1][page] = bad
            c = _twin_decode(shape, 0, exps, positions, table, q, k, v, kc8, vc8, cos, sin, w8, w16, table_for_launch=broken)
            assert bool(torch.isnan(c["out"][1]).all())
            assert torch.equal(_bits(c["out"][0]), _bits(c["ref"][0])) and torch.equal(_bits(c["out"][2]), _bits(c["ref"][2]))
            _check_pools(c, table, [(0, 65, 66), (2, 127, 128)], exps, (page, use_ws))            # nothing of slot 1
            if use_ws:                                        # the refused sequence left the workspace alone
                c = _twin_decode(shape, 0, exps, positions, table, q, k, v, kc8, vc8, cos, sin, w8, w16)
                assert torch.equal(_bits(c["out"]), _bits(c["ref"]))
    q, k, v, kc8, vc8 = _ragged_inputs(shape, exps, True)
    rows, positions = [n for n, _ in SEGMENTS], [p for _, p in SEGMENTS]
    table = _assignment([(p + n + PAGE - 1) // PAGE for n, p in SEGMENTS], 9)
    order = (3, 4, 1)
    for page in (0, 3):                                       # segment 4: a page it reads, one it appends to
        broken = [list(r) for r in table]
        broken[4][page] = bad
        c = _twin_ragged(0, exps, order, rows, positions, table, q, k, v, kc8, vc8, cos, sin, table_for_launch=broken)
        assert bool(torch.isnan(c["out"][c["seg"][4]]).all())
        for j in (3, 1):
            assert torch.equal(_bits(c["out"][c["seg"][j]]), _bits(c["ref"][c["seg"][j]]))
        _check_pools(c, table, [(j, positions[j], positions[j] + rows[j]) for j in (3, 1)], exps, page)


def test_wrappers_refuse_what_they_can_see():
    shape, exps = SHAPES[0], (0, 0)
    heads, kvh, hd = shape
    q, k, v, kc8, vc8 = _decode_inputs(shape, exps, True)
    cos, sin = _tables(hd)
    pos = torch.zeros(3, dtype=torch.long, device=DEV)
    table = _dev_table(_assignment((MAX_PAGES,) * 3, 5))
    _, kp8 = _pool8(kc8, [[-1] * MAX_PAGES] * 3)
    f8, f16 = _ops().rope_attn_decode_paged_f8, _ops().rope_attn_decode_paged
    with pytest.raises(ValueError):
        f8(q, k, v, cos, sin, pos, table, _deq(kp8, 0), _deq(kp8, 0), None, 0, 0, 0)                # fp16 pools
    with pytest.raises(ValueError):
        f16(q, k, v, cos, sin, pos, table, kp8, kp8.clone(), None, 0)                               # uint8 pools
    with pytest.raises(ValueError):
        f8(q, k, v, cos, sin, pos, table, kp8, kp8.clone(), None, 0, 8, 0)                          # exponent
    with pytest.raises(ValueError):
        f8(q, k, v, cos, sin, pos, table, kp8, kp8.clone(), None, 0, 0, -9)
    with pytest.raises(ValueError):
        f8(q, k, v, cos, sin, pos, table, kp8[:, :, :32].contiguous(), kp8.clone(), None, 0, 0, 0)  # not 64-row pages
