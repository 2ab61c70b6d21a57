"""Attention inputs whose softmax is peaked, tied or uniform instead of nearly flat, for the host models
(tests/test_attn_hard_cases_host.py) and the launches (tests/test_gpu_attn_hard_cases.py).  CPU only.

A builder returns a Case for ONE head group: the query heads of a KV head (GROUP of them: q and 1.25 q, so the group
shares its winner), `rows` new rows behind `pos` cached ones (a decode step is rows == 1), and what row `i` of the chunk
must come out as.  K is given as the cache holds it -- rotated; for an fp8 cache (exps = (k_exp, v_exp)) K and V hold the
values the stored bytes mean, so quantising them is exact.  Keys row i does not see (below its window, chunk rows behind
it) score 60 along its query: a mask that lets one through hands it the whole output.

    one_winner   one key scores 40, the rest 0 +- noise: out == V[t*] bit for bit (every other weight <= e^-30)
    two_winners  two keys of the same bytes score 40: out == fp16((V[t1] + V[t2]) / 2) bit for bit, V integers
    uniform      every visible key scores the same (K = 0, or one row repeated): the mean of integer V rows within one
                 fp16 ulp (sums exact in fp32, l == n exactly)
    hard         score distributions a trained model has and randn has not, compared with float64 attention"""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np
import torch

from tests.test_chunk_attn_host import exact_attention, first_key

GROUP = 2
GROUP_SCALES = (1.0, 1.25)
HARD_KINDS = ("sharp8", "asc", "desc", "sink", "saw", "big")
WIN, POISON, GAP = 40.0, 60.0, 30.0


class Case(NamedTuple):
    q: torch.Tensor          # (rows, GROUP, hd) fp16, before the rotary embedding
    k_new: torch.Tensor      # (rows, hd) fp16, before the rotary embedding
    v_new: torch.Tensor      # (rows, hd) fp16
    K: torch.Tensor          # (pos, hd) fp16, the cached rows (rotated)
    V: torch.Tensor          # (pos, hd) fp16
    expected: torch.Tensor   # bits: (GROUP, hd) fp16; ulp: (GROUP, hd) float64; bound: (rows, GROUP, hd) float64
    pos: int
    window: int
    i: Optional[int]         # the chunk row `expected` is about (bound: every row)
    rule: str                # "bits" | "ulp" | "bound"
    vmax: Optional[torch.Tensor]     # bound: (rows,) max|v| over each row's keys
    K_all: torch.Tensor      # (pos + rows, hd) every key as stored after the launch
    V_all: torch.Tensor


@functools.lru_cache(maxsize=None)
def _tables(hd, max_len):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)


def tables(hd, max_len):
    """cos / sin as every test of the launches builds them -> two (max_len, hd) float32 (a row does not depend on
    max_len: the leading rows of one table per head size)"""
    cos, sin = _tables(hd, max(8192, max_len))
    return cos[:max_len], sin[:max_len]


def rope(x, cos, sin):
    """the eager formula the launches restate (_rope of tests/test_gpu_chunk_attn.py): x (..., hd) fp16, cos / sin
    broadcastable rows of the tables"""
    d = x.shape[-1] // 2
    rot = torch.cat([-x[..., d:], x[..., :d]], -1)
    return (x.float() * cos + rot.float() * sin).to(x.dtype)


def turn64(x, delta):
    """x (hd,) float64 turned by `delta` (m,) positions of the rotary embedding -> (m, hd) float64"""
    hd = x.shape[-1]
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float64) / hd))
    ang = torch.as_tensor(delta, dtype=torch.float64)[:, None] * inv[None, :]
    c, s = torch.cat([ang.cos(), ang.cos()], -1), torch.cat([ang.sin(), ang.sin()], -1)
    rot = torch.cat([-x[hd // 2:], x[:hd // 2]], -1)
    return x * c + rot * s


def store(x, e):
    """what a cache keeps of fp16 x: x itself, or at fp8 exponent e the value of its e4m3fn byte (paged_attn.quant_f8 /
    dequant_f8 restated)"""
    if e is None:
        return x
    b = (x.float() * 2.0 ** -int(e)).clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    return (b.float() * 2.0 ** int(e)).to(torch.float16)


def q_scale_for(exps):
    """the size of q at which the winner's row, 40 sqrt(hd) / |q|^2 q, sits inside the e4m3 range at k_exp"""
    return 1.0 if exps is None or exps[0] > -6 else 16.0


def v_scale_for(exps):
    return 1.0 if exps is None else 2.0 ** (exps[1] + 3)


@functools.lru_cache(maxsize=64)
def _drawn(seed, shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


class _Rng:
    """seeded draws; the normal ones are kept (read only), since a sweep over t* asks for the same ones again and again"""

    def __init__(self, seed):
        self.seed, self.calls = seed, 0
        self.g = torch.Generator().manual_seed(seed)

    def randn(self, *shape):
        self.calls += 1
        return _drawn((self.seed * 16 + self.calls) % (2 ** 62), shape)


def _gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return _Rng(seed)


def _randn(g, *shape):
    return g.randn(*shape)


def _visible(pos, i, window):
    p = pos + i
    return first_key(p, window), p


def _scores64(qr, K_all):
    """float64 scores of every key against the rotated fp16 query heads qr (GROUP, hd) -> (n, GROUP)"""
    hd = qr.shape[-1]
    return K_all.double() @ qr.double().T * float(np.float32(1.0 / math.sqrt(hd)))


def _queries(g, hd, rows, exps):
    q0 = (q_scale_for(exps) * _randn(g, rows, hd)).to(torch.float16)
    return torch.stack([(sc * q0.float()).to(torch.float16) for sc in GROUP_SCALES], 1)


def along(q, pos, i, s, g, exps=None):
    """key rows whose score against row i's rotated query (head 0 of the group) is s[t], on top of 0.1 * randn noise (in
    units of 1 / the size of q): K[t] = noise[t] + s[t] sqrt(hd) / |q|^2 q, rounded to fp16.  Chunk row i's own key is
    built the same way from the unrotated q, every other chunk row's from the direction turned back to its position.
    -> K (pos, hd), k_new (rows, hd)"""
    rows, _, hd = q.shape
    n = pos + rows
    s = torch.as_tensor(s, dtype=torch.float64)
    cos, sin = tables(hd, n)
    p = pos + i
    qr = rope(q[i, 0], cos[p], sin[p]).double()
    c = math.sqrt(hd) / float(qr @ qr)
    noise = 0.1 / q_scale_for(exps) * _randn(g, n, hd)
    K = (noise[:pos] + s[:pos, None] * c * qr).to(torch.float16)
    d = c * turn64(qr, -(pos + torch.arange(rows, dtype=torch.float64)))
    qi = q[i, 0].double()
    d[i] = math.sqrt(hd) / float(qi @ qi) * qi
    k_new = (noise[pos:] + s[pos:, None] * d).to(torch.float16)
    return K, k_new


def _all_keys(K, k_new, pos, exps):
    rows, hd = k_new.shape
    cos, sin = tables(hd, pos + rows)
    e = None if exps is None else exps[0]
    return torch.cat([store(K, e), store(rope(k_new, cos[pos:], sin[pos:]), e)])


def _rotated(q, pos, i):
    hd = q.shape[-1]
    cos, sin = tables(hd, pos + i + 1)
    return rope(q[i], cos[pos + i], sin[pos + i])


def _masked_scores(n, a, p, inside):
    s = torch.full((n,), POISON, dtype=torch.float64)
    s[a:p + 1] = inside
    return s


def _check_gap(q, pos, i, K_all, winners, a, p):
    """in float64, on the keys as stored: every winner beats every other visible key by >= GAP for every head"""
    sc = _scores64(_rotated(q, pos, i), K_all)[a:p + 1]
    w = torch.zeros(p + 1 - a, dtype=torch.bool)
    w[[t - a for t in winners]] = True
    if (~w).any():
        gap = sc[w].min(0).values - sc[~w].max(0).values
        assert bool((gap >= GAP).all()), f"gap {gap.tolist()} at pos {pos} row {i} winners {winners}"
    return sc[w]


def one_winner_sweep(hd, pos, t_stars, rows=1, i=0, window=0, exps=None, seed=0):
    """one_winner for every t* of t_stars: the cases share q, the noise and V and differ in the one planted row (built
    once for all: the keys at score 0 and the keys at score 40, case t* takes row t* of the second)"""
    a, p = _visible(pos, i, window)
    n, key = pos + rows, (1, hd, pos, rows, i, window, seed, 0 if exps is None else 100 + 16 * exps[0] + exps[1])
    g = _gen(*key)
    q = _queries(g, hd, rows, exps)
    K0, k0 = along(q, pos, i, _masked_scores(n, a, p, 0.0), g, exps)
    v = (v_scale_for(exps) * _randn(g, n, hd)).to(torch.float16)
    # no zero among the stored values: next to weights of e^-30 the sign of a zero is anybody's
    v[store(v, None if exps is None else exps[1]) == 0] = 2.0 ** (-24 if exps is None else exps[1] - 9)
    g = _gen(*key)                                   # the same draws again: the same noise under the winners
    _queries(g, hd, rows, exps)
    K1, k1 = along(q, pos, i, _masked_scores(n, a, p, WIN), g, exps)
    all0, all1 = _all_keys(K0, k0, pos, exps), _all_keys(K1, k1, pos, exps)
    V_all = store(v, None if exps is None else exps[1])
    # in float64, on the keys as stored: the winner beats every other visible key by >= GAP for every head
    qr = _rotated(q, pos, i)
    sc0, sc1 = _scores64(qr, all0)[a:p + 1], _scores64(qr, all1)[a:p + 1]
    cases = []
    for t in t_stars:
        assert a <= t <= p
        if p > a:
            rest = torch.cat([sc0[:t - a], sc0[t - a + 1:]]).max(0).values
            assert bool((sc1[t - a] - rest >= GAP).all()), f"gap {(sc1[t - a] - rest).tolist()} at pos {pos} row {i} t* {t}"
        K_all, k_new = all0.clone(), k0.clone()
        K_all[t] = all1[t]
        if t >= pos:
            k_new[t - pos] = k1[t - pos]
        cases.append(Case(q, k_new, v[pos:], K_all[:pos], V_all[:pos], V_all[t].expand(GROUP, hd).contiguous(), pos, window,
                          i, "bits", None, K_all, V_all))
    return cases


def one_winner(hd, pos, t_star, rows=1, i=0, window=0, exps=None, seed=0):
    return one_winner_sweep(hd, pos, [t_star], rows, i, window, exps, seed)[0]


def _integers(g, n, hd, exps):
    v = torch.randint(-8, 9, (n, hd), generator=g.g).double()
    return v, (1.0 if exps is None else 2.0 ** exps[1])


def two_winners(hd, pos, t1, t2, rows=1, i=0, window=0, exps=None, seed=0):
    """t1 a cached row, t2 behind it: a cached row of the same bytes, or a new row -- then row t1 is planted as the
    rotated new row the launch itself appends"""
    a, p = _visible(pos, i, window)
    assert a <= t1 < t2 <= p and t1 < pos
    g = _gen(2, hd, pos, rows, i, window, seed, t1, t2, 0 if exps is None else 100 + 16 * exps[0] + exps[1])
    q = _queries(g, hd, rows, exps)
    s = _masked_scores(pos + rows, a, p, 0.0)
    s[t1] = s[t2] = WIN
    K, k_new = along(q, pos, i, s, g, exps)
    K_all = _all_keys(K, k_new, pos, exps)
    K_all[t1] = K_all[t2]
    v, unit = _integers(g, pos + rows, hd, exps)
    tie = v[t1] + v[t2] == 0                         # a sum of exactly 0 would leave the sign to the e^-40 rows
    v[t2] = torch.where(tie, torch.where(v[t2] == 0, torch.ones(hd, dtype=torch.float64), v[t2] - v[t2].sign()), v[t2])
    V_all = (v * unit).to(torch.float16)
    sc = _check_gap(q, pos, i, K_all, [t1, t2], a, p)
    assert torch.equal(sc[0], sc[1])
    expected = ((V_all[t1].double() + V_all[t2].double()) / 2).to(torch.float16)
    return Case(q, k_new, V_all[pos:], K_all[:pos], V_all[:pos], expected.expand(GROUP, hd).contiguous(), pos, window, i,
                "bits", None, K_all, V_all)


def uniform(hd, pos, identical=False, rows=1, i=0, window=0, exps=None, seed=0):
    """row i sees n keys: pos + i + 1 without a window.  identical: every visible row is the row the launch appends for
    chunk row i (score about 37), which therefore has to be the only visible new row: i == 0"""
    assert pos >= 0 and (not identical or i == 0)
    a, p = _visible(pos, i, window)
    g = _gen(3, hd, pos, identical, rows, i, window, seed, 0 if exps is None else 100 + 16 * exps[0] + exps[1])
    q = _queries(g, hd, rows, exps)
    s = _masked_scores(pos + rows, a, p, 37.0 if identical else 0.0)
    K, k_new = along(q, pos, i, s, g, exps)
    if not identical:
        K[a:pos] = 0
        k_new[max(a - pos, 0):i + 1] = 0
    K_all = _all_keys(K, k_new, pos, exps)
    if identical:
        K_all[a:pos] = K_all[pos]
    v, unit = _integers(g, pos + rows, hd, exps)
    V_all = (v * unit).to(torch.float16)
    sc = _scores64(_rotated(q, pos, i), K_all)[a:p + 1]
    assert bool((sc == sc[0]).all()) and (identical or bool((sc == 0).all()))
    expected = V_all[a:p + 1].double().mean(0)
    return Case(q, k_new, V_all[pos:], K_all[:pos], V_all[:pos], expected.expand(GROUP, hd).contiguous(), pos, window, i,
                "ulp", None, K_all, V_all)


def hard(kind, hd, pos, rows=1, window=0, exps=None, seed=0):
    """the kinds are built along the LAST row's query (it sees every key); every row is compared with float64.
    A decode case (rows == 1) whose exact answer rounds to fp16 by more than 0.5 u on its own is drawn again: the decode
    family's bound grants the output rounding 0.5 u (0.5 ulp(out) is up to |out| / max|v| u, so an answer next to max|v| just
    above a power of two takes more), and such a case would measure its own rounding and not the launch"""
    for draw in range(16):
        case = _hard(kind, hd, pos, rows, window, exps, seed + 1000 * draw)
        own = (case.expected.to(torch.float16).double() - case.expected).abs().amax(-1) / (case.vmax[:, None] * 2.0 ** -11)
        if rows > 1 or float(own.max()) <= 0.5:
            return case
    raise AssertionError(f"{kind} at {pos}: no draw whose own rounding stays within 0.5 u")


def _hard(kind, hd, pos, rows, window, exps, seed):
    n, i = pos + rows, rows - 1
    g = _gen(4, HARD_KINDS.index(kind), hd, pos, rows, window, seed, 0 if exps is None else 100 + 16 * exps[0] + exps[1])
    q = _queries(g, hd, rows, exps)
    t = torch.arange(n, dtype=torch.float64)
    if kind == "sharp8":
        K = (8.0 / q_scale_for(exps) * _randn(g, pos, hd)).to(torch.float16)
        k_new = (8.0 / q_scale_for(exps) * _randn(g, rows, hd)).to(torch.float16)
    else:
        if kind == "asc":
            s = torch.linspace(-30, 30, n, dtype=torch.float64)
        elif kind == "desc":
            s = torch.linspace(30, -30, n, dtype=torch.float64)
        elif kind == "sink":
            s = torch.zeros(n, dtype=torch.float64)
            s[first_key(pos + i, window)] = 12.0
        elif kind == "saw":
            s = 20.0 * (t % 64) / 64
        else:
            s = 80.0 * (2 * torch.rand(n, generator=g.g, dtype=torch.float64) - 1)
        K, k_new = along(q, pos, i, s, g, exps)
    v = (v_scale_for(exps) * _randn(g, n, hd)).to(torch.float16)
    K_all = _all_keys(K, k_new, pos, exps)
    V_all = store(v, None if exps is None else exps[1])
    cos, sin = tables(hd, n)
    qr = rope(q, cos[pos:, None], sin[pos:, None])
    expected = torch.empty(rows, GROUP, hd, dtype=torch.float64)
    for h in range(GROUP):
        e, vmax = exact_attention(qr[:, h].numpy(), K_all.numpy(), V_all.numpy(), pos, window, 1.0 / math.sqrt(hd))
        expected[:, h] = torch.from_numpy(e)
    return Case(q, k_new, v[pos:], K_all[:pos], V_all[:pos], expected, pos, window, None, "bound", torch.from_numpy(vmax),
                K_all, V_all)


def ulp16(x):
    """the spacing of fp16 at |x| (float64 tensor in, float64 out): 2^(floor(log2 |x|) - 10), 2^-24 below 2^-14"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -14))) - 10)
