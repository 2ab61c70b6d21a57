"""The hard attention cases (tests/attn_hard_cases.py) without a GPU: a CPU model of the decode launch's arithmetic
(rope_attn_decode_kernel, csrc/decode_glue.hip; the batched, paged and fp8 launches are instantiations of it), the bound
the decode family is held to on the device, and both models -- this one and model_attention of
tests/test_chunk_attn_host.py for the chunk launches -- exact on the constructed cases and inside their bounds on the hard
score distributions.  A model outside its bound means the derivation is wrong: it is mended here, never fitted to a kernel.

Error unit, as in the chunk tests: u = 2^-11 * max|v| over the keys a row attends to."""
import math

import numpy as np
import pytest
import torch

from tests import attn_hard_cases as H
from tests.test_chunk_attn_host import BOUND_U, CHUNKS, error_in_u, first_key, model_attention

SPLITS, SPLIT_FROM_POS = 8, 256          # kSplits, kSplitFromPos
HDS = (64, 128)


def BOUND_DECODE_U(n):
    """0.5 u is the one rounding of the output to fp16 in the accounting of the chunk bound (half an fp16 ulp of a value
    below max|v|; it is 0.5 ulp(out) / u, between |out| / (2 max|v|) and |out| / max|v|, so an output next to max|v| and just
    above a power of two would take up to 1 u by rounding alone -- none of the cases here does).  P stays in fp32 in these
    launches, so what is left is the fp32 arithmetic: a running sum over n keys grows by at most one
    rounding, 2^-24 relative, per key -- n * 2^-24 of a value below max|v| in the worst case, which is n / 8192 u (the
    numerator and the denominator do not both reach it: lane groups and splits cut the chains to n / NG keys, and the
    merges add NG + 8 more roundings).  The scores (<= 128 products, |s| <= 80: an absolute error of 80 * 2^-21, the
    argument scaling inside __expf included) move a weight by less than 4e-5 relative, 0.01 u, inside the slack."""
    return 0.5 + n / 8192.0


def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _lane_group_states(q32, k32, v32, t_lo, t_hi, ng, lpk):
    """the lane groups of one workgroup over [t_lo, t_hi): group g takes t_lo + g + ng j; attn::score (8 fmas per lane,
    then the butterfly over the group's lanes) and attn::update key by key -> m, l (ng,), acc (ng, hd)"""
    hd = q32.shape[0]
    m = np.full(ng, -np.inf, dtype=np.float32)
    l = np.zeros(ng, dtype=np.float32)
    acc = np.zeros((ng, hd), dtype=np.float32)
    lanes = np.arange(lpk)
    with np.errstate(invalid="ignore", over="ignore"):
        for t0 in range(t_lo, t_hi, ng):
            t = t0 + np.arange(ng)
            ok = t < t_hi
            tc = np.where(ok, t, t_lo)
            k, v = k32[tc].reshape(ng, lpk, 8), v32[tc]
            s = np.zeros((ng, lpk), dtype=np.float32)
            for d in range(8):
                s = _fma(np.broadcast_to(q32.reshape(lpk, 8)[:, d], (ng, lpk)), k[:, :, d], s)
            o = 1
            while o < lpk:
                s = (s + s[:, lanes ^ o]).astype(np.float32)
                o *= 2
            s = s[:, 0]
            mn = np.maximum(m, s)
            c = np.exp((m - mn).astype(np.float32)).astype(np.float32)
            p = np.exp((s - mn).astype(np.float32)).astype(np.float32)
            l2 = _fma(l, c, p)
            acc2 = _fma(acc, c[:, None], (p[:, None] * v).astype(np.float32))
            m, l, acc = np.where(ok, mn, m), np.where(ok, l2, l), np.where(ok[:, None], acc2, acc)
    return m, l, acc


def _merge_states(m, l, o):
    """attn::merge_states over the states in order: m, l (N,), o (N, hd) -> (M, L, O (hd,)); a state that saw no key
    (m = -inf) has weight 0, N such states give (-inf, 0, 0)"""
    M = np.float32(m.max())
    L, O = np.float32(0), np.zeros(o.shape[1], dtype=np.float32)
    for i in range(len(m)):
        w = np.float32(0) if np.isneginf(m[i]) else np.exp(np.float32(m[i] - M)).astype(np.float32)
        L = _fma(np.float32(l[i]), w, L)
        O = _fma(o[i], w, O)
    return M, L, O


def model_decode(qr, k, v, window, split):
    """the decode launch's arithmetic for one head: qr (hd,) the rotated fp16 query at position pos = len(k) - 1, k / v
    (pos + 1, hd) the rows [0, pos] as stored.  q scaled in fp32, NG = 256 / (hd / 8) lane groups striding over
    [t_lo, t_hi), the groups' states merged; split: 8 contiguous chunks of ceil((pos + 1 - first) / 8) keys, each a
    workgroup, their states merged (from position 256 on, as the launch does), empty ones included -> (hd,) fp16"""
    k32, v32 = (np.asarray(t, dtype=np.float16).astype(np.float32) for t in (k, v))
    pos, hd = k32.shape[0] - 1, k32.shape[1]
    lpk = hd // 8
    ng = 256 // lpk
    q32 = (np.asarray(qr, dtype=np.float16).astype(np.float32) * np.float32(1.0 / math.sqrt(hd))).astype(np.float32)
    first = first_key(pos, window)
    split = split and pos >= SPLIT_FROM_POS
    chunk = (pos - first + SPLITS) // SPLITS if split else pos + 1 - first
    states = []
    for s in range(SPLITS if split else 1):
        t_lo = first + s * chunk
        t_hi = min(pos + 1, t_lo + chunk)
        states.append(_merge_states(*_lane_group_states(q32, k32, v32, t_lo, t_hi, ng, lpk)))
    if not split:
        _, L, O = states[0]
    else:
        _, L, O = _merge_states(np.array([s[0] for s in states]), np.array([s[1] for s in states]),
                                np.stack([s[2] for s in states]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (O / L).astype(np.float16)


def _decode_out(case, split):
    """(GROUP, hd) fp16: the decode model on a one-row case"""
    qr = H._rotated(case.q, case.pos, 0).numpy()
    return np.stack([model_decode(qr[h], case.K_all.numpy(), case.V_all.numpy(), case.window, split)
                     for h in range(H.GROUP)])


def _chunk_out(case):
    """(rows, GROUP, hd) fp16: the chunk model on a case"""
    hd, rows = case.q.shape[-1], case.q.shape[0]
    cos, sin = H.tables(hd, case.pos + rows)
    qr = H.rope(case.q, cos[case.pos:, None], sin[case.pos:, None]).numpy()
    return np.stack([model_attention(qr[:, h], case.K_all.numpy(), case.V_all.numpy(), case.pos, case.window,
                                     1.0 / math.sqrt(hd)) for h in range(H.GROUP)], 1)


def _check(case, got):
    """got (GROUP, hd) fp16 for the case's row against its rule"""
    if case.rule == "bits":
        assert np.array_equal(got.view(np.int16), case.expected.numpy().view(np.int16))
    else:
        e = case.expected
        assert bool(((torch.from_numpy(got.astype(np.float64)) - e).abs() <= H.ulp16(e)).all())


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("n,window", [(301, 0), (4101, 0), (301, 100), (4101, 1000)])
@pytest.mark.parametrize("split", [False, True])
def test_decode_model_stays_inside_the_bound_on_the_hard_kinds(hd, n, window, split):
    """the cases of the GPU test (window 0 and a window), both modes"""
    keys = n - first_key(n - 1, window)
    for kind in H.HARD_KINDS:
        case = H.hard(kind, hd, n - 1, window=window)
        got = _decode_out(case, split)
        e = max(error_in_u(got[h][None], case.expected[0, h].numpy()[None], case.vmax.numpy()) for h in range(H.GROUP))
        print(f"decode model hd {hd} n {n} window {window} split {split} {kind}: {e:.3f} u (bound {BOUND_DECODE_U(keys):.3f})")
        assert e <= BOUND_DECODE_U(keys), kind


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("window", [0, 16])
def test_chunk_model_stays_inside_its_bound_on_the_hard_kinds(hd, window):
    for kind in H.HARD_KINDS:
        for rows, pos in CHUNKS:
            case = H.hard(kind, hd, pos, rows=rows, window=window)
            got = _chunk_out(case)
            e = max(error_in_u(got[:, h], case.expected[:, h].numpy(), case.vmax.numpy()) for h in range(H.GROUP))
            print(f"chunk model hd {hd} window {window} rows {rows} pos {pos} {kind}: {e:.3f} u (bound {BOUND_U})")
            assert e <= BOUND_U, (kind, rows, pos)


def _constructed(hd, pos, window=0):
    """one-row cases at a position: winners at the edges of what the row sees, pairs of winners, both uniform variants"""
    a = first_key(pos, window)
    cases = [H.one_winner(hd, pos, t, window=window) for t in sorted({a, (a + pos) // 2, max(a, pos - 1), pos})]
    if pos > a:
        cases += [H.two_winners(hd, pos, a, pos, window=window)]
    if pos > a + 1:
        cases += [H.two_winners(hd, pos, a, pos - 1, window=window)]
    return cases + [H.uniform(hd, pos, identical=x, window=window) for x in (False, True)]


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("pos,window", [(0, 0), (1, 0), (64, 0), (300, 0), (300, 5), (300, 1), (4100, 0)])
def test_decode_model_is_exact_on_the_constructed_cases(hd, pos, window):
    for case in _constructed(hd, pos, window):
        for split in (False, True):
            _check(case, _decode_out(case, split))


@pytest.mark.parametrize("hd", HDS)
@pytest.mark.parametrize("window", [0, 16])
def test_chunk_model_is_exact_on_the_constructed_cases(hd, window):
    for rows, pos in CHUNKS:
        for i in sorted({0, rows // 2, rows - 1}):
            a, p = first_key(pos + i, window), pos + i
            cases = [H.one_winner(hd, pos, t, rows, i, window) for t in sorted({a, max(a, min(pos - 1, p)), p})]
            if a < pos:
                cases += [H.two_winners(hd, pos, a, p, rows, i, window)]
            cases += [H.uniform(hd, pos, False, rows, i, window)]
            if i == 0:
                cases += [H.uniform(hd, pos, True, rows, i, window)]
            for case in cases:
                _check(case, _chunk_out(case)[i])


def test_the_builders_keep_their_promises():
    """the planted rows are where they are said to be, and the fp8 cases hold only bytes' values"""
    for exps in (None, (0, 0), (-8, -8), (7, 7)):
        c = H.one_winner(64, 130, 77, exps=exps)
        assert torch.equal(c.expected[0], c.V_all[77]) and c.K.shape == (130, 64) and c.k_new.shape == (1, 64)
        c = H.two_winners(64, 130, 63, 64, exps=exps)
        assert torch.equal(c.K[63], c.K[64]) and not torch.equal(c.K[63], c.K[62])
        c = H.two_winners(64, 130, 5, 130, exps=exps)
        assert torch.equal(c.K[5], c.K_all[130])
        if exps is not None:
            assert torch.equal(H.store(c.K, exps[0]), c.K) and torch.equal(H.store(c.V, exps[1]), c.V)
    # a window leaves poison below it: the first visible key of (300, window 5) is 296
    c = H.one_winner(128, 300, 296, window=5)
    sc = H._scores64(H._rotated(c.q, 300, 0), c.K_all)
    assert bool((sc[:296] > 50).all()) and bool((sc[297:] < 10).all())
