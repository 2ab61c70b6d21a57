"""Every attention launch on the inputs of tests/attn_hard_cases.py: peaked, tied and uniform softmax instead of the nearly
flat one of randn rows, where a lost or doubled key moves the output by less than the tolerance.

    one winner    out == V[t*] bit for bit, every key the winner once (lane-group stride, rounds of four keys, the eight
                  split chunks, splits that walk nothing, page edges, the fp8 conversion, the window's edges)
    two winners   on either side of a seam: out == fp16((V[t1] + V[t2]) / 2) bit for bit
    uniform       the mean of n integer rows within one fp16 ulp: a row dropped or doubled is tens of ulps
    hard kinds    against float64 attention, the decode family inside BOUND_DECODE_U(keys), the chunk family inside BOUND_U
                  (both derived on the CPU: tests/test_attn_hard_cases_host.py, tests/test_chunk_attn_host.py), and the
                  bit identities between the launches again on these inputs

A sequence of a batched launch carries two cases (one per KV head), so a sweep is a handful of launches; everything is
compared on the device and brought over once per test.  The paged launches run on a shuffled table inside a poisoned
allocation with a guard page on either side (the harness of tests/test_gpu_paged_attn.py), and every launch's cache is
compared, whole, with what it must be afterwards.

Worst errors seen on an MI355X: profiles/attn_hard_cases.txt."""
import functools
import types

import pytest
import torch

from tests import attn_hard_cases as H
from tests.test_attn_hard_cases_host import BOUND_DECODE_U, SPLITS
from tests.test_chunk_attn_host import BOUND_U, CHUNKS, first_key
from tests.test_gpu_paged_attn import SEGMENTS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((4, 2, 64), (4, 2, 128))               # heads, kv_heads, head_dim: both lane-group widths, a group of two
PAGE, MAX_LEN = 64, 384
EXPS = ((0, 0), (-8, -8), (7, 7))                # (k_exp, v_exp)
POISON16, POISON8 = 777.0, 0x7E
POSITIONS = (0, 1, 63, 64, 127, 128, 255, 256, 257, 300)


def _ops():
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.batch_decode  # noqa: F401
    import quip_for_all_amd.chunk_attn  # noqa: F401
    import quip_for_all_amd.paged_attn  # noqa: F401
    import quip_for_all_amd.ragged_attn  # noqa: F401
    return torch.ops.quip_lib


@functools.lru_cache(maxsize=None)
def _tables(hd, max_len):
    cos, sin = H.tables(hd, max_len)
    return cos.contiguous().to(DEV), sin.contiguous().to(DEV)


def _ws(batch, heads, hd):
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    return rope_attn_batched_workspace(batch, heads, hd, DEV)


# ---- fp8 bytes on the device, for values that are bytes' values already (the builders' promise) ------------------------------
@functools.lru_cache(maxsize=None)
def _lut(e):
    """byte -> fp16 value at exponent e (NaN codes -> NaN); and the finite values sorted, with their codes"""
    lut = (torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).float() * 2.0 ** e).to(torch.float16)
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f and c != 0x80], dtype=torch.uint8)
    vals, order = lut[codes.long()].float().sort()
    return lut.to(DEV), vals.to(DEV), codes[order].to(DEV)


def _bytes(x, e):
    """fp16 values that are e4m3 values at exponent e -> their bytes (-0 as +0), and whether every one was"""
    lut, vals, codes = _lut(e)
    b = codes[torch.bucketize(x.float(), vals).clamp(max=vals.numel() - 1)]
    return b, (lut[b.long()] == x).all()


def _deq(b, e):
    return _lut(e)[0][b.long()]


# ---- one comparison per test --------------------------------------------------------------------------------------------------
class _Tally:
    """what the launches gave against what they must give, kept on the device: add() takes values that pass when <= 1,
    finish() brings all of them over at once, fails on the first label beyond 1 (or NaN) and returns the worst per label"""

    def __init__(self):
        self.items = []

    def add(self, label, value):
        self.items.append((label, value.double().reshape(-1)))

    def same(self, label, a, b):
        """bit for bit (fp16 through its bits: NaN == NaN, -0 != 0)"""
        if a.dtype == torch.float16:
            a, b = a.view(torch.int16), b.view(torch.int16)
        assert a.shape == b.shape, label
        self.add(label, (a != b).any().double() * 2)

    def true(self, label, flag):
        self.add(label, (~flag).double() * 2)

    def finish(self):
        flat = torch.cat([v for _, v in self.items]).cpu()          # the one synchronisation
        worst, at = {}, 0
        for label, v in self.items:
            x = flat[at:at + v.numel()]
            at += v.numel()
            bad = (~(x <= 1)).nonzero().flatten().tolist()
            assert not bad, f"{label}: {len(bad)} of {x.numel()} beyond the rule, first at {bad[:8]}, worst {float(x.max()):.3f}"
            worst[label] = max(worst.get(label, 0.0), float(x.max()))
        return worst


def _measure(rule, out, expected, vmax=None, bound=None):
    """(.., heads, hd) against the rule -> (.., heads), passing when <= 1"""
    if rule == "bits":
        return (out.view(torch.int16) != expected.view(torch.int16)).any(-1).double() * 2
    err = (out.double() - expected).abs()
    if rule == "ulp":
        return (err / H.ulp16(expected)).amax(-1)
    return err.amax(-1) / (vmax * 2.0 ** -11) / bound


# ---- the decode family: rows == 1 cases, two per sequence ---------------------------------------------------------------------
def _pack(shape, cases, max_len=MAX_LEN, exps=None):
    """cases -> the operands of a batched launch, a sequence for every two cases at one position (one per KV head; an odd
    one out goes in twice), the caches as they must be after it, and the expectation; everything on the device"""
    heads, kvh, hd = shape
    assert heads == kvh * H.GROUP
    by_pos = {}
    for c in cases:
        by_pos.setdefault(c.pos, []).append(c)
    cases = [c for group in by_pos.values() for c in group + group[-1:] * (len(group) % kvh)]
    B = len(cases) // kvh
    rule, window = cases[0].rule, cases[0].window
    kc, vc = (torch.zeros(B, kvh, max_len, hd, dtype=torch.float16) for _ in range(2))
    ak, av = kc.clone(), vc.clone()
    for n, c in enumerate(cases):
        b, j = divmod(n, kvh)
        assert c.q.shape[0] == 1 and c.pos == cases[kvh * b].pos and c.window == window and c.rule == rule
        kc[b, j, :c.pos], vc[b, j, :c.pos] = c.K, c.V
        ak[b, j, :c.pos + 1], av[b, j, :c.pos + 1] = c.K_all, c.V_all
    grp = lambda f: torch.stack([torch.stack([f(cases[kvh * b + j]) for j in range(kvh)]) for b in range(B)])  # noqa: E731
    P = types.SimpleNamespace(B=B, rule=rule, window=window, exps=exps, max_len=max_len,
                              positions=[cases[kvh * b].pos for b in range(B)])
    P.q = grp(lambda c: c.q[0]).reshape(B, heads, hd).to(DEV)
    P.k, P.v = grp(lambda c: c.k_new[0]).to(DEV), grp(lambda c: c.v_new[0]).to(DEV)
    P.kc, P.vc, P.ak, P.av = kc.to(DEV), vc.to(DEV), ak.to(DEV), av.to(DEV)
    P.pos = torch.tensor(P.positions, dtype=torch.long, device=DEV)
    P.vmax = P.bound = None
    if rule == "bound":
        P.expected = grp(lambda c: c.expected[0]).reshape(B, heads, hd).to(DEV)
        P.vmax = grp(lambda c: c.vmax[0].expand(H.GROUP)).reshape(B, heads).to(DEV)
        keys = [p + 1 - first_key(p, window) for p in P.positions]
        P.bound = torch.tensor([BOUND_DECODE_U(n) for n in keys], dtype=torch.float64, device=DEV)[:, None]
    else:
        P.expected = grp(lambda c: c.expected).reshape(B, heads, hd).to(DEV)
    return P


def _check_out(tally, label, P, out):
    tally.add(label, _measure(P.rule, out, P.expected, P.vmax, P.bound))


def _batched(tally, label, shape, P, use_ws):
    """rope_attn_decode_batched on clones of the pack's caches -> out; the caches afterwards are the expected ones"""
    cos, sin = _tables(shape[2], P.max_len)
    kc, vc = P.kc.clone(), P.vc.clone()
    ws = _ws(P.B, shape[0], shape[2]) if use_ws else None
    out = _ops().rope_attn_decode_batched(P.q, P.k, P.v, cos, sin, P.pos, kc, vc, ws, P.window)
    _check_out(tally, label, P, out)
    tally.same(label + " caches", torch.stack([kc, vc]), torch.stack([P.ak, P.av]))
    if use_ws:
        tally.true(label + " counters", ~ws[-4 * P.B * shape[0]:].any())
    return out


def _single(tally, label, shape, P, b, use_ws):
    """rope_attn_decode on sequence b of the pack"""
    from quip_for_all_amd.register_lib import rope_attn_workspace
    cos, sin = _tables(shape[2], P.max_len)
    kc, vc = P.kc[b].clone(), P.vc[b].clone()
    ws = rope_attn_workspace(shape[0], shape[2], DEV) if use_ws else None
    out = _ops().rope_attn_decode(P.q[b], P.k[b], P.v[b], cos, sin, P.pos[b:b + 1], kc, vc, ws, P.window)
    tally.add(label, _measure(P.rule, out, P.expected[b], None if P.vmax is None else P.vmax[b],
                              None if P.bound is None else P.bound[b]))
    tally.same(label + " caches", torch.stack([kc, vc]), torch.stack([P.ak[b], P.av[b]]))
    return out


def _table(B, max_pages, seed):
    """every page owned, shuffled: (B, max_pages) int32 on the device"""
    g = torch.Generator().manual_seed(seed)
    return torch.randperm(B * max_pages, generator=g).view(B, max_pages).to(torch.int32).to(DEV)


def _pool(contig, table, poison):
    """the poisoned allocation with a guard page on either side, holding contig (B, kvh, L, hd) through the table"""
    B, kvh, L, hd = contig.shape
    mp = L // PAGE
    big = torch.full((B * mp + 2, kvh, PAGE, hd), poison, dtype=contig.dtype, device=DEV)
    big[1 + table.flatten().long()] = contig.view(B, kvh, mp, PAGE, hd).permute(0, 2, 1, 3, 4).reshape(B * mp, kvh, PAGE, hd)
    return big


def _paged(tally, label, shape, P, use_ws, seed=5):
    """rope_attn_decode_paged (P.exps None) or _f8 on the pack's caches behind a shuffled table"""
    from quip_for_all_amd.paged_attn import gather
    cos, sin = _tables(shape[2], P.max_len)
    table = _table(P.B, P.max_len // PAGE, seed)
    ws = _ws(P.B, shape[0], shape[2]) if use_ws else None
    if P.exps is None:
        bigk, bigv = _pool(P.kc, table, POISON16), _pool(P.vc, table, POISON16)
        out = _ops().rope_attn_decode_paged(P.q, P.k, P.v, cos, sin, P.pos, table, bigk[1:-1], bigv[1:-1], ws, P.window)
        tally.same(label + " pools", torch.stack([gather(bigk[1:-1], table), gather(bigv[1:-1], table)]), torch.stack([P.ak, P.av]))
        tally.true(label + " guards", (torch.stack([bigk[0], bigk[-1], bigv[0], bigv[-1]]) == POISON16).all())
    else:
        (k8, okk), (v8, okv) = _bytes(P.kc, P.exps[0]), _bytes(P.vc, P.exps[1])
        tally.true(label + " representable", okk & okv)
        bigk, bigv = _pool(k8, table, POISON8), _pool(v8, table, POISON8)
        out = _ops().rope_attn_decode_paged_f8(P.q, P.k, P.v, cos, sin, P.pos, table, bigk[1:-1], bigv[1:-1], ws, P.window,
                                               P.exps[0], P.exps[1])
        # the pools afterwards, by value (a zero may be stored with either sign): the expected rows, the new one as stored
        tally.true(label + " pools", (_deq(gather(bigk[1:-1], table), P.exps[0]) == P.ak).all()
                   & (_deq(gather(bigv[1:-1], table), P.exps[1]) == P.av).all())
        tally.true(label + " guards", (torch.stack([bigk[0], bigk[-1], bigv[0], bigv[-1]]) == POISON8).all())
    _check_out(tally, label, P, out)
    return out


def _decode_family(tally, shape, make, max_len=MAX_LEN, contiguous=True):
    """make(exps) -> cases.  The batched launch and both paged launches, each with and without the workspace (split mode
    from position 256 on), fp8 at every exponent pair -> {label: out} of the fp16 launches"""
    outs = {}
    P = _pack(shape, make(None), max_len)
    for use_ws in (False, True):
        mode = "split" if use_ws else "one"
        if contiguous:
            outs["batched " + mode] = _batched(tally, "batched " + mode, shape, P, use_ws)
        outs["paged " + mode] = _paged(tally, "paged " + mode, shape, P, use_ws)
    for exps in EXPS:
        P8 = _pack(shape, make(exps), max_len, exps)
        for use_ws in (False, True):
            _paged(tally, f"paged f8 {exps} " + ("split" if use_ws else "one"), shape, P8, use_ws)
    return P, outs


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", (0, 100))
@pytest.mark.parametrize("pos", POSITIONS)
def test_every_key_is_the_winner_once(shape, window, pos):
    tally = _Tally()
    ts = range(first_key(pos, window), pos + 1)
    _decode_family(tally, shape, lambda exps: H.one_winner_sweep(shape[2], pos, ts, window=window, exps=exps))
    tally.finish()


def _split_edges(pos, first=0):
    chunk = (pos - first + SPLITS) // SPLITS
    return [first + s * chunk for s in range(SPLITS + 1)]


@pytest.mark.parametrize("shape", SHAPES)
def test_winners_at_the_edges_of_the_eight_splits(shape):
    """position 1030, split mode: the first and last two rows of each split's chunk, both sides of every multiple of 64 up
    to 256, row 0 and the new row"""
    pos, max_len = 1030, 1088
    edges = _split_edges(pos)
    ts = {0, pos}
    for lo, hi in zip(edges, edges[1:]):
        ts |= {lo, lo + 1, min(hi, pos + 1) - 2, min(hi, pos + 1) - 1}
    for m in (64, 128, 192, 256):
        ts |= {m - 1, m}
    ts = sorted(ts)
    assert len(ts) >= 32 and edges[1] == 129
    tally = _Tally()
    P = _pack(shape, H.one_winner_sweep(shape[2], pos, ts), max_len)
    _batched(tally, "batched split", shape, P, True)
    _paged(tally, "paged split", shape, P, True)
    for exps in EXPS:
        _paged(tally, f"paged f8 {exps} split", shape, _pack(shape, H.one_winner_sweep(shape[2], pos, ts, exps=exps), max_len, exps), True)
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", (5, 1))
def test_every_row_of_a_short_window_wins_in_split_mode(shape, window):
    """position 300: the eight splits share 5 keys or 1, those that walk nothing are merged with weight 0"""
    tally = _Tally()
    ts = range(first_key(300, window), 301)
    _decode_family(tally, shape, lambda exps: H.one_winner_sweep(shape[2], 300, ts, window=window, exps=exps))
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
def test_single_sequence_launch_on_a_sample_of_winners(shape):
    pairs = [(0, 0), (1, 0), (1, 1), (63, 31), (64, 63), (64, 64), (127, 0), (128, 127), (255, 128), (256, 0), (256, 32),
             (256, 255), (256, 256), (257, 33), (257, 256), (300, 0), (300, 37), (300, 38), (300, 63), (300, 64), (300, 75),
             (300, 76), (300, 151), (300, 152), (300, 265), (300, 266), (300, 299), (300, 300)]
    windowed = [(300, 100, 201), (300, 100, 213), (300, 100, 214), (300, 100, 300), (257, 100, 158), (257, 100, 170),
                (64, 100, 0), (300, 5, 296), (300, 5, 298), (300, 5, 300), (300, 1, 300), (128, 100, 29), (128, 100, 128)]
    assert len(pairs) + len(windowed) >= 40
    tally = _Tally()
    for pos, w, t in [(p, 0, t) for p, t in pairs] + windowed:
        other = (t + pos) // 2 if w == 0 else max(t - 1, first_key(pos, w))          # KV head 1 has a winner of its own
        P = _pack(shape, H.one_winner_sweep(shape[2], pos, [t, other], window=w))
        for use_ws in (False, True):
            _single(tally, "single " + ("split" if use_ws else "one"), shape, P, 0, use_ws)
    tally.finish()


def _seams(hd, exps):
    """pairs of winners: a lane-group wrap (t, t + NG) and a round of four (t, t + 4 NG), from a split's first key too;
    the edges of the split chunks at position 300 (38 keys each); the page edge; a cached row with the new row"""
    ng = 256 // (hd // 8)
    pairs = [(300, 0, ng), (300, 5, 5 + ng), (300, ng - 1, 2 * ng - 1), (300, 0, 4 * ng), (300, 3, 3 + 4 * ng),
             (300, 38, 38 + ng), (300, 76 + 1, 76 + 1 + ng), (300, 37, 38), (300, 75, 76), (300, 265, 266), (300, 63, 64),
             (300, 255, 256), (300, 0, 300), (300, 299, 300), (300, 100, 300), (130, 63, 64), (130, 0, ng), (255, 7, 7 + 4 * ng),
             (130, 129, 130), (64, 63, 64), (64, 0, 64), (1, 0, 1), (255, 127, 128), (256, 255, 256), (256, 31, 32)]
    return [H.two_winners(hd, pos, t1, t2, exps=exps) for pos, t1, t2 in pairs]


def _window_seams(hd, exps):
    ng = 256 // (hd // 8)
    pairs = ((201, 201 + ng), (201, 300), (213, 214), (255, 256), (202, 202 + (4 if hd == 128 else 3) * ng), (299, 300))
    return [H.two_winners(hd, 300, t1, t2, window=100, exps=exps) for t1, t2 in pairs]


@pytest.mark.parametrize("shape", SHAPES)
def test_two_winners_on_either_side_of_each_seam(shape):
    tally = _Tally()
    P, _ = _decode_family(tally, shape, lambda exps: _seams(shape[2], exps))
    table = _table(P.B, MAX_LEN // PAGE, 5).cpu()              # the page edge is one between two non-adjacent pages
    assert all(abs(int(r[1]) - int(r[0])) > 1 for r in table)
    for b in range(P.B):
        for use_ws in (False, True):
            _single(tally, "single " + ("split" if use_ws else "one"), shape, P, b, use_ws)
    # in a window: the wrap counts from the window's first key (100 keys: the fourth key of a round only at head size 128)
    _decode_family(tally, shape, lambda exps: _window_seams(shape[2], exps))
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("identical", (False, True))
def test_uniform_softmax_counts_every_key_once(shape, identical):
    hd = shape[2]
    tally = _Tally()
    ns = (1, 2, 64, 65, 257, 301)
    P, _ = _decode_family(tally, shape, lambda exps: [H.uniform(hd, n - 1, identical, exps=exps, seed=s) for n in ns for s in (0, 1)])
    for b in range(P.B):
        for use_ws in (False, True):
            _single(tally, "single " + ("split" if use_ws else "one"), shape, P, b, use_ws)
    # a window of 100 (257 and 301 keys behind: 100 are counted), and the short windows in split mode
    for window in (100, 5, 1):
        P, _ = _decode_family(tally, shape, lambda exps: [H.uniform(hd, n - 1, identical, window=window, exps=exps, seed=s)
                                                          for n in ns for s in (0, 1)])
        for b in (3, 5):
            for use_ws in (False, True):
                _single(tally, f"single window {window} " + ("split" if use_ws else "one"), shape, P, b, use_ws)
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
def test_uniform_softmax_over_4101_keys(shape):
    """several ulps per row still: 8 / 4101 against an fp16 ulp of at most 2^-8 for a mean below 8"""
    tally = _Tally()
    for identical in (False, True):
        P = _pack(shape, [H.uniform(shape[2], 4100, identical, seed=s) for s in (0, 1)], 4160)
        for use_ws in (False, True):
            _single(tally, "single " + ("split" if use_ws else "one"), shape, P, 0, use_ws)
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pos,window", [(300, 0), (300, 100), (4100, 0), (4100, 1000)])
def test_hard_distributions_against_float64(shape, pos, window):
    """every kind on every launch of the decode family, both modes, inside BOUND_DECODE_U(keys); fp8 against float64 on the
    pool's values after the launch, with the same bound; and batched == single, paged == contiguous, bit for bit"""
    hd = shape[2]
    max_len = MAX_LEN if pos < MAX_LEN else 4160
    tally = _Tally()
    P, outs = _decode_family(tally, shape, lambda exps: [H.hard(kind, hd, pos, window=window, exps=exps) for kind in H.HARD_KINDS],
                             max_len)
    for mode in ("one", "split"):
        tally.same(f"paged == batched ({mode})", outs["paged " + mode], outs["batched " + mode])
        single = torch.stack([_single(tally, "single " + mode, shape, P, b, mode == "split") for b in range(P.B)])
        tally.same(f"batched == single ({mode})", outs["batched " + mode], single)
    worst = tally.finish()
    for label, w in sorted(worst.items()):
        if label.split()[-1] in ("one", "split"):
            keys = pos + 1 - first_key(pos, window)
            print(f"hd {hd} pos {pos} window {window} {label}: {w * BOUND_DECODE_U(keys):.3f} u (bound {BOUND_DECODE_U(keys):.3f})")
    # per kind, on the batched launch in split mode
    e = (_measure("bound", outs["batched split"], P.expected, P.vmax, P.bound) * P.bound).reshape(-1, H.GROUP).amax(1).tolist()
    print(f"hd {hd} pos {pos} window {window} batched split per kind: " + ", ".join(f"{k} {x:.3f}" for k, x in zip(H.HARD_KINDS, e)))


# ---- the chunk family: cases with `rows` new rows -----------------------------------------------------------------------------
def _chunk_operands(shape, pair):
    """a pair of cases on one chunk (one per KV head) -> q (rows, heads, hd), k, v (rows, kvh, hd), caches (kvh, MAX_LEN, hd)
    before and after, on the CPU"""
    heads, kvh, hd = shape
    a, b = pair
    rows, pos = a.q.shape[0], a.pos
    assert b.q.shape[0] == rows and b.pos == pos and a.window == b.window
    q = torch.cat([a.q, b.q], 1)
    k, v = torch.stack([a.k_new, b.k_new], 1), torch.stack([a.v_new, b.v_new], 1)
    kc, vc = (torch.zeros(kvh, MAX_LEN, hd, dtype=torch.float16) for _ in range(2))
    ak, av = kc.clone(), vc.clone()
    for j, c in enumerate(pair):
        kc[j, :pos], vc[j, :pos] = c.K, c.V
        ak[j, :pos + rows], av[j, :pos + rows] = c.K_all, c.V_all
    return q, k, v, kc, vc, ak, av


def _chunk_expect(tally, label, shape, pair, out, bound=BOUND_U):
    """out (rows, heads, hd) of a pair's chunk against each case's rule"""
    for j, c in enumerate(pair):
        o = out[:, j * H.GROUP:(j + 1) * H.GROUP]
        if c.rule == "bound":
            tally.add(label, _measure("bound", o, c.expected.to(DEV), c.vmax.to(DEV)[:, None], bound))
        else:
            tally.add(label, _measure(c.rule, o[c.i], c.expected.to(DEV)))


def _chunk(tally, label, shape, pair):
    cos, sin = _tables(shape[2], MAX_LEN)
    q, k, v, kc, vc, ak, av = (t.to(DEV) for t in _chunk_operands(shape, pair))
    pos = torch.tensor([pair[0].pos], dtype=torch.long, device=DEV)
    out = _ops().rope_attn_chunk(q, k, v, cos, sin, pos, kc, vc, pair[0].window)
    _chunk_expect(tally, label, shape, pair, out)
    tally.same(label + " caches", torch.stack([kc, vc]), torch.stack([ak, av]))
    return out


def _ragged(tally, shape, pairs, exps=None, contiguous=True, seed=7):
    """up to 32 pairs as the segments of one launch, slot b segment b: rope_attn_ragged and rope_attn_ragged_paged on the
    same operands (exps None), or rope_attn_ragged_paged_f8 -> the out rows of the (last) launch"""
    from quip_for_all_amd.paged_attn import gather
    heads, kvh, hd = shape
    cos, sin = _tables(hd, MAX_LEN)
    ops = [_chunk_operands(shape, p) for p in pairs]
    q, k, v = (torch.cat([o[n] for o in ops]).to(DEV) for n in range(3))
    kc, vc, ak, av = (torch.stack([o[n] for o in ops]).to(DEV) for n in range(3, 7))
    B = len(pairs)
    pos = torch.tensor([p[0].pos for p in pairs], dtype=torch.long, device=DEV)
    seg_slot, seg_rows, window = list(range(B)), [p[0].q.shape[0] for p in pairs], pairs[0][0].window
    off = [0]
    for n in seg_rows:
        off.append(off[-1] + n)

    def expect(label, out):
        for b, pair in enumerate(pairs):
            _chunk_expect(tally, label, shape, pair, out[off[b]:off[b + 1]])

    table = _table(B, MAX_LEN // PAGE, seed)
    if exps is None:
        outs = {}
        if contiguous:
            kc2, vc2 = kc.clone(), vc.clone()
            outs["ragged"] = _ops().rope_attn_ragged(q, k, v, cos, sin, pos, seg_slot, seg_rows, kc2, vc2, window)
            expect("ragged", outs["ragged"])
            tally.same("ragged caches", torch.stack([kc2, vc2]), torch.stack([ak, av]))
        bigk, bigv = _pool(kc, table, POISON16), _pool(vc, table, POISON16)
        outs["ragged paged"] = _ops().rope_attn_ragged_paged(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, bigk[1:-1],
                                                             bigv[1:-1], window)
        expect("ragged paged", outs["ragged paged"])
        tally.same("ragged paged pools", torch.stack([gather(bigk[1:-1], table), gather(bigv[1:-1], table)]), torch.stack([ak, av]))
        tally.true("ragged paged guards", (torch.stack([bigk[0], bigk[-1], bigv[0], bigv[-1]]) == POISON16).all())
        if contiguous:
            tally.same("ragged paged == ragged", outs["ragged paged"], outs["ragged"])
        return outs
    (k8, okk), (v8, okv) = _bytes(kc, exps[0]), _bytes(vc, exps[1])
    label = f"ragged paged f8 {exps}"
    tally.true(label + " representable", okk & okv)
    bigk, bigv = _pool(k8, table, POISON8), _pool(v8, table, POISON8)
    out = _ops().rope_attn_ragged_paged_f8(q, k, v, cos, sin, pos, seg_slot, seg_rows, table, bigk[1:-1], bigv[1:-1], window,
                                           exps[0], exps[1])
    expect(label, out)
    tally.true(label + " pools", (_deq(gather(bigk[1:-1], table), exps[0]) == ak).all()
               & (_deq(gather(bigv[1:-1], table), exps[1]) == av).all())
    tally.true(label + " guards", (torch.stack([bigk[0], bigk[-1], bigv[0], bigv[-1]]) == POISON8).all())
    return {label: out}


def _winner_rows(rows, pos, window):
    """(chunk row, t*): rows {first, middle, last}, each against its first visible key, the last cached row, itself and both
    sides of every multiple of 64 in between"""
    pairs = []
    for i in sorted({0, rows // 2, rows - 1}):
        a, p = first_key(pos + i, window), pos + i
        ts = {a, p} | ({pos - 1} if pos - 1 >= a else set())
        for m in range(64, p + 1, 64):
            ts |= {t for t in (m - 1, m) if a <= t <= p}
        pairs += [(i, t) for t in sorted(ts)]
    return pairs


def _winner_pairs(hd, segments, window, exps):
    """for every segment, its (row, t*) cases two by two (KV head 0 walks them forwards, KV head 1 backwards)"""
    pairs = []
    for rows, pos in segments:
        by_row = {}
        for i, t in _winner_rows(rows, pos, window):
            by_row.setdefault(i, []).append(t)
        cases = [c for i, ts in by_row.items() for c in H.one_winner_sweep(hd, pos, ts, rows, i, window, exps)]
        pairs += list(zip(cases, reversed(cases)))[:(len(cases) + 1) // 2]
    return pairs


def _in_launches(pairs):
    return [pairs[n:n + 32] for n in range(0, len(pairs), 32)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", (0, 16))
def test_chunk_rows_with_one_winner(shape, window):
    """rope_attn_chunk and rope_attn_ragged on CHUNKS, the paged launches on the SEGMENTS of their own tests"""
    tally = _Tally()
    pairs = _winner_pairs(shape[2], CHUNKS, window, None)
    for pair in pairs:
        _chunk(tally, "chunk", shape, pair)
    for group in _in_launches(pairs):
        _ragged(tally, shape, group)
    for group in _in_launches(_winner_pairs(shape[2], SEGMENTS, window, None)):
        _ragged(tally, shape, group)
    for exps in EXPS:
        for group in _in_launches(_winner_pairs(shape[2], SEGMENTS, window, exps)):
            _ragged(tally, shape, group, exps)
    tally.finish()


def _chunk_seams(hd, window, exps):
    """two winners for chunk row i, ((rows, pos), i, t1, t2): on either side of a key tile's edge (both cached; cached and in
    the chunk), a cached row with a chunk row -- an earlier one and the row itself; with a window, inside it"""
    spec = {0: [((70, 130), 69, 63, 64), ((70, 130), 69, 127, 128), ((70, 130), 69, 129, 130), ((70, 130), 69, 0, 199),
                ((70, 130), 30, 100, 160), ((70, 130), 0, 129, 130), ((64, 300), 63, 255, 256), ((64, 300), 20, 299, 320),
                ((64, 300), 63, 0, 363), ((33, 61), 32, 60, 61), ((33, 61), 10, 60, 64), ((5, 3), 4, 2, 7), ((5, 3), 1, 0, 4)],
            16: [((70, 130), 5, 127, 128), ((70, 130), 5, 129, 130), ((70, 130), 5, 120, 135), ((64, 300), 10, 299, 310),
                 ((64, 300), 14, 299, 300), ((33, 61), 3, 60, 64), ((33, 61), 3, 49, 63), ((5, 3), 4, 2, 7), ((5, 3), 1, 0, 4)]}
    return [H.two_winners(hd, pos, t1, t2, rows, i, window, exps) for (rows, pos), i, t1, t2 in spec[window]]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", (0, 16))
def test_chunk_rows_with_two_winners(shape, window):
    tally = _Tally()
    mk = lambda exps: [(c, c) for c in _chunk_seams(shape[2], window, exps)]  # noqa: E731
    pairs = mk(None)
    for pair in pairs:
        _chunk(tally, "chunk", shape, pair)
    _ragged(tally, shape, pairs)
    for exps in EXPS:
        _ragged(tally, shape, mk(exps), exps)
    tally.finish()


def _chunk_uniform(hd, identical, exps):
    """n keys for the row that is asked: the last row of a chunk of up to 70 rows (the zero variant), the first row of a
    chunk of three (the repeated row: it is the row the launch appends for that chunk row)"""
    cases = []
    for n in (1, 2, 64, 65, 257, 301):
        for s in (0, 1):
            if identical:
                cases.append(H.uniform(hd, n - 1, True, rows=3, i=0, exps=exps, seed=s))
            else:
                rows = min(n, 70)
                cases.append(H.uniform(hd, n - rows, False, rows=rows, i=rows - 1, exps=exps, seed=s))
    return list(zip(cases[::2], cases[1::2]))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("identical", (False, True))
def test_chunk_rows_with_a_uniform_softmax(shape, identical):
    tally = _Tally()
    pairs = _chunk_uniform(shape[2], identical, None)
    for pair in pairs:
        _chunk(tally, "chunk", shape, pair)
    _ragged(tally, shape, pairs)
    for exps in EXPS:
        _ragged(tally, shape, _chunk_uniform(shape[2], identical, exps), exps)
    tally.finish()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", (0, 16))
def test_chunk_launches_on_the_hard_distributions(shape, window):
    """every kind at CHUNKS, every row against float64 inside BOUND_U; the chunk in several launches gives the bits of the
    chunk in one; ragged == chunk and ragged paged == ragged, bit for bit"""
    hd = shape[2]
    cos, sin = _tables(hd, MAX_LEN)
    tally = _Tally()
    mk = lambda exps: [tuple(H.hard(kind, hd, pos, rows, window, exps, seed=j) for j in range(2))  # noqa: E731
                       for kind in H.HARD_KINDS for rows, pos in CHUNKS]
    pairs = mk(None)
    whole = [_chunk(tally, "chunk", shape, pair) for pair in pairs]
    outs = _ragged(tally, shape, pairs)
    tally.same("ragged == chunk", outs["ragged"], torch.cat(whole))
    for pair, one in zip(pairs, whole):
        rows, pos = pair[0].q.shape[0], pair[0].pos
        if rows < 33:
            continue
        q, k, v, kc, vc, ak, av = (t.to(DEV) for t in _chunk_operands(shape, pair))
        for step in (7, 32):
            kc2, vc2 = kc.clone(), vc.clone()
            parts = [_ops().rope_attn_chunk(q[r:r + step], k[r:r + step], v[r:r + step], cos, sin,
                                            torch.tensor([pos + r], dtype=torch.long, device=DEV), kc2, vc2, window)
                     for r in range(0, rows, step)]
            tally.same(f"chunk in steps of {step}", torch.cat(parts), one)
            tally.same(f"chunk in steps of {step} caches", torch.stack([kc2, vc2]), torch.stack([ak, av]))
    for exps in EXPS:
        _ragged(tally, shape, mk(exps), exps)
    worst = tally.finish()
    for label, w in sorted(worst.items()):
        if label in ("chunk", "ragged", "ragged paged") or label.endswith(")"):
            print(f"hd {hd} window {window} {label}: {w * BOUND_U:.3f} u (bound {BOUND_U})")
