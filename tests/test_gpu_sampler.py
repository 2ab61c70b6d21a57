"""quip_lib::sample_step (csrc/sample_rows.hip.h) on the device against the float64 restatement of its function
(sampler.sample_step_ref), draw by draw.

Draw acceptance: the op's token g passes iff its float64 interval [lo_g, hi_g) comes within DELTA * Z of u * Z, DELTA =
2^-18 being the bound on the relative error of any prefix mass that the kernel's header derives (no exclusions).
p-cut acceptance: a (row, setting) whose oracle margin min_j |mass above class j - p Z_k| / Z_k is <= DELTA is left out of
the `kept` and draw comparisons -- the cut itself is undecided there.  The cap on what a test may leave out is twice the
oracle's own share on this grid, which never exceeds the issue's 6 %: checked on the CPU with the oracle alone, 8 of the
1800 random items (0.44 %) and 2 of the 216 constructed ones are left out at DELTA = 2^-18, at most 2 in any test, so a
test may leave out 4 items, or 1 % of its items where that is more.  Everything else is exact: `kept`, greedy rows
against argmax_step_batched, and the invariances (row of a batch / alone, misaligned / aligned, call after call)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1), (3, 7), (2, 255), (5, 257), (4, 1024), (3, 2049), (2, 8193), (2, 32003), (1, 152064), (2, 70001)]
GRID = [(T, k, p) for T in (0.7, 1.0) for p in (0.5, 0.9, 0.95, 1.0) for k in (0, 1, 40)]
SCALES = (1, 4, 16)


def _cap(items):
    """how many items a test may leave out: twice the oracle's largest count in any test here (2), or 1 % (twice its share
    of the grid, 0.44 %, rounded up) where that is more; below the issue's 6 % for every test of this file (>= 72 items)"""
    return max(4, items // 100)


def _S():
    from quip_for_all_amd import sampler
    return sampler


def _op(logits, T, k, p, seed, pos, want_kept=True):
    """one launch on `logits` (rows, n) as it lies; the parameters are lists (rows,) -> (tok, pos after, kept) lists"""
    _S()
    rows = logits.shape[0]
    def dev(v, dt):
        return torch.tensor(v, dtype=dt, device=DEV)
    tok = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    post = dev(pos, torch.int64)
    kept = torch.full((rows,), -7, dtype=torch.int32, device=DEV) if want_kept else None
    torch.ops.quip_lib.sample_step(logits, dev(T, torch.float32), dev(k, torch.int32), dev(p, torch.float32),
                                   dev(seed, torch.int64), tok, post, kept)
    torch.cuda.synchronize()
    return tok.tolist(), post.tolist(), (kept.tolist() if want_kept else None)


def _check_rows(x_cpu, tok, kept, T, k, p, seed, pos, stats):
    """the acceptance rules on every row of one launch; stats = [items, left out]"""
    S = _S()
    n = x_cpu.shape[1]
    for r in range(x_cpu.shape[0]):
        d = S.sample_dist_ref(x_cpu[r], T[r], k[r], p[r])
        stats[0] += 1
        assert 0 <= tok[r] < n, (r, tok[r])
        if d["margin"] <= S.DELTA:
            stats[1] += 1
            continue
        assert kept[r] == d["kept"], (r, T[r], k[r], p[r], kept[r], d["kept"], d["margin"])
        assert S.sample_accepts(d, tok[r], seed[r], pos[r]), (r, T[r], k[r], p[r], seed[r], pos[r], tok[r],
                                                              S.sample_draw_ref(d, seed[r], pos[r]))


def _randn(rows, n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, n, generator=g) * scale).to(torch.float16)


@pytest.mark.parametrize("rows,n", SHAPES)
def test_random_rows_against_the_oracle(rows, n):
    stats = [0, 0]
    for scale in SCALES:
        x = _randn(rows, n, scale, 1000 * scale + n)
        xd = x.to(DEV)
        for c, (T, k, p) in enumerate(GRID):
            seed = [977 * c + 31 * r + n for r in range(rows)]
            pos = [(5 * c + r) % 97 for r in range(rows)]
            tok, post, kept = _op(xd, [T] * rows, [k] * rows, [p] * rows, seed, pos)
            assert post == [c_ + 1 for c_ in pos]
            _check_rows(x, tok, kept, [T] * rows, [k] * rows, [p] * rows, seed, pos, stats)
    print(f"({rows}, {n}): {stats[1]} of {stats[0]} items left out (p-cut margin <= delta)")
    assert stats[1] <= _cap(stats[0]) <= 0.06 * stats[0], stats


CONSTRUCTED_N = (257, 2049, 32003)
CONSTRUCTED_GRID = [(1.0, k, p) for k in (0, 1, 40) for p in (0.5, 0.9, 1.0)]
KINDS = ["all_equal", "one_winner", "two_winners", "tie_at_k", "minus_inf_padding", "a_nan", "all_nan", "plus_inf"]


@functools.lru_cache(maxsize=None)
def _constructed(kind, n):
    x = _randn(1, n, 2.0, n + len(kind))[0]
    if kind == "all_equal":
        x[:] = 1.5
    elif kind == "one_winner":
        x[n // 3] = float(x.max()) + 30.0
    elif kind == "two_winners":
        x[n // 5] = x[n - 2] = float(x.max()) + 1.0
    elif kind == "tie_at_k":                     # places 31 .. 50 hold one value: k = 40 keeps 50 tokens
        order = torch.argsort(x.float(), descending=True)
        x[order[30:50]] = x[order[30]].clone()
    elif kind == "minus_inf_padding":
        x[n - n // 3:] = -float("inf")
        x[1] = -float("inf")
    elif kind == "a_nan":
        x[n // 2] = float("nan")
        x[0] = float("nan")
    elif kind == "all_nan":
        x[:] = float("nan")
    elif kind == "plus_inf":
        x[n // 4] = x[n // 2] = float("inf")
    return x.reshape(1, n)


@pytest.mark.parametrize("n", CONSTRUCTED_N)
def test_constructed_rows_against_the_oracle(n):
    x = torch.cat([_constructed(kind, n) for kind in KINDS])
    xd = x.to(DEV)
    rows = len(KINDS)
    stats = [0, 0]
    for c, (T, k, p) in enumerate(CONSTRUCTED_GRID):
        seed = [13 * c + r for r in range(rows)]
        pos = [c + 3 * r for r in range(rows)]
        tok, post, kept = _op(xd, [T] * rows, [k] * rows, [p] * rows, seed, pos)
        assert post == [c_ + 1 for c_ in pos]
        _check_rows(x, tok, kept, [T] * rows, [k] * rows, [p] * rows, seed, pos, stats)
        if p == 1.0:                                                     # k-only: kept is exact, whatever the margin
            got = dict(zip(KINDS, kept))                                 # (the oracle agreed above; these are by construction)
            assert got["all_equal"] == n
            if k == 0:
                assert (got["one_winner"], got["minus_inf_padding"], got["a_nan"]) == (n, n - n // 3 - 1, n - 2)
            if k == 1:
                assert (got["one_winner"], got["two_winners"]) == (1, 2)
            if k == 40:
                assert got["tie_at_k"] == 50
        assert tok[KINDS.index("all_nan")] == 0 and tok[KINDS.index("plus_inf")] == n // 4
        if k == 1:
            assert tok[KINDS.index("one_winner")] == n // 3 and tok[KINDS.index("two_winners")] in (n // 5, n - 2)
    assert stats[1] <= _cap(stats[0]) <= 0.06 * stats[0], stats


def test_all_equal_row_draws_every_index_by_rank():
    """one class of n tokens: the draw is the rank floor(u n) exactly (the weights are all 2^40 units), over several rounds
    of 8192 elements and a ragged tail"""
    S = _S()
    n, rows = 20011, 64
    x = torch.full((rows, n), -3.25, dtype=torch.float16, device=DEV)
    seed, pos = list(range(100, 100 + rows)), [7] * rows
    tok, _, kept = _op(x, [0.9] * rows, [0] * rows, [1.0] * rows, seed, pos)
    assert kept == [n] * rows
    assert tok == [int(S.sample_uniform(s, 7) * n) for s in seed]


@pytest.mark.parametrize("rows,n", SHAPES)
def test_greedy_rows_are_argmax_step_batched_bit_for_bit(rows, n):
    """T = 0 (and T < 0, NaN) on random rows with ties, and the rows whose maximum is not finite at T = 1"""
    import quip_for_all_amd.batch_decode  # noqa: F401  (defines argmax_step_batched)
    x = (_randn(rows, n, 2.0, n) * 4).round() / 4                       # quarter steps: tied maxima
    special = torch.stack([torch.full((n,), float("nan"), dtype=torch.float16),
                           torch.full((n,), -float("inf"), dtype=torch.float16),
                           _randn(1, n, 1.0, 5)[0].index_fill_(0, torch.tensor([n - 1, n // 2]), float("inf")),
                           _randn(1, n, 1.0, 6)[0].index_fill_(0, torch.tensor([n // 3]), float("nan"))])
    xs = torch.cat([x, special]).to(DEV)
    R = rows + 4
    T = [[0.0, -1.0, float("nan")][r % 3] for r in range(rows)] + [1.0, 1.0, 1.0, 0.0]
    pos = [3 + r for r in range(R)]
    tok, post, kept = _op(xs, T, [40] * R, [0.9] * R, list(range(R)), pos)
    t2 = torch.full((R,), -7, dtype=torch.int64, device=DEV)
    p2 = torch.tensor(pos, dtype=torch.int64, device=DEV)
    torch.ops.quip_lib.argmax_step_batched(xs, t2, p2)
    assert tok == t2.tolist() and post == p2.tolist() and kept == [1] * R
    assert tok[rows] == 0 and tok[rows + 1] == 0 and tok[rows + 2] == n // 2


@pytest.mark.parametrize("rows,n", [(5, 257), (3, 2049), (2, 32003), (3, 7), (2, 70001)])
def test_a_row_of_a_batch_has_the_bits_of_a_call_on_that_row_alone(rows, n):
    x = _randn(rows, n, 4.0, n + 1).to(DEV)
    T, k, p = [0.7, 1.0, 0.9, 1.3, 0.0][:rows], [0, 40, 5, 0, 3][:rows], [0.9, 1.0, 0.5, 0.95, 0.9][:rows]
    seed, pos = [11 + r for r in range(rows)], [r * 9 for r in range(rows)]
    tok, post, kept = _op(x, T, k, p, seed, pos)
    for r in range(rows):
        t1, p1, k1 = _op(x[r:r + 1].clone(), T[r:r + 1], k[r:r + 1], p[r:r + 1], seed[r:r + 1], pos[r:r + 1])
        assert (t1[0], p1[0], k1[0]) == (tok[r], post[r], kept[r]), r
    # ... and of the same row at another index, among other rows, without the kept output
    perm = list(reversed(range(rows)))
    t3, _, none = _op(x[perm].contiguous(), [T[i] for i in perm], [k[i] for i in perm], [p[i] for i in perm],
                      [seed[i] for i in perm], [pos[i] for i in perm], want_kept=False)
    assert none is None and t3 == [tok[i] for i in perm]


@pytest.mark.parametrize("n", [7, 257, 2049, 32003])
def test_a_misaligned_row_has_the_bits_of_an_aligned_copy(n):
    x = _randn(2, n, 4.0, n + 2).to(DEV)
    buf = torch.zeros(2 * n + 16, dtype=torch.float16, device=DEV)
    args = ([0.8, 1.0], [40, 0], [0.9, 0.95], [5, 6], [17, 0])
    want = _op(x, *args)
    for off in (1, 3, 4, 7):                                          # 2, 6, 8 and 14 bytes past a 16-byte boundary
        view = buf[off:off + 2 * n].view(2, n)
        view.copy_(x)
        assert view.data_ptr() % 16 == (2 * off) % 16 and view.is_contiguous()
        assert _op(view, *args) == want, off


def test_two_calls_in_a_row():
    x = _randn(3, 2049, 4.0, 9).to(DEV)
    args = ([0.8, 1.0, 0.6], [40, 0, 7], [0.9, 0.95, 1.0], [5, 6, 7])
    first = _op(x, *args, [4, 0, 90])
    assert _op(x, *args, [4, 0, 90]) == first                           # the same call again: the same bits
    # the counter advances on the device: the second of two calls in a row is a call at position + 1
    _S()
    tok = torch.zeros(3, dtype=torch.int64, device=DEV)
    pos = torch.tensor([4, 0, 90], dtype=torch.int64, device=DEV)
    par = [torch.tensor(v, dtype=dt, device=DEV) for v, dt in zip(args, (torch.float32, torch.int32, torch.float32, torch.int64))]
    torch.ops.quip_lib.sample_step(x, *par, tok, pos)
    assert tok.tolist() == first[0] and pos.tolist() == [5, 1, 91]
    torch.ops.quip_lib.sample_step(x, *par, tok, pos)
    assert pos.tolist() == [6, 2, 92] and tok.tolist() == _op(x, *args, [5, 1, 91])[0]


def test_4096_seeds_of_one_row_in_one_launch_draw_by_draw():
    S = _S()
    n, R = 2049, 4096
    row = _randn(1, n, 3.0, 77)
    T, k, p = 0.9, 40, 0.9
    d = S.sample_dist_ref(row[0], T, k, p)
    assert d["margin"] > 16 * S.DELTA and d["kept"] >= 5
    x = row.expand(R, n).contiguous().to(DEV)
    tok, _, kept = _op(x, [T] * R, [k] * R, [p] * R, list(range(R)), [12] * R)
    assert kept == [d["kept"]] * R
    ref = [S.sample_draw_ref(d, s, 12) for s in range(R)]
    bad = [s for s in range(R) if not S.sample_accepts(d, tok[s], s, 12)]
    assert not bad, bad[:8]
    print(f"{sum(tok[s] != ref[s] for s in range(R))} of {R} draws differ from the oracle's own token (u Z within delta Z of a boundary)")
    counts = np.bincount(np.array(tok), minlength=n)
    q = np.diff(np.concatenate([[0.0], d["cum"]])) / d["Z"]
    for t, qt in zip(d["order"].tolist(), q.tolist()):
        assert abs(counts[t] - R * qt) <= 5 * np.sqrt(R * qt * (1 - qt)) + 3, (t, counts[t], R * qt)
    assert counts.sum() == counts[d["order"]].sum()


def test_out_of_range_parameters_read_as_off_or_greedy():
    S = _S()
    n = 1024
    x = _randn(1, n, 2.0, 3)
    rows = [(1.0, -5, 1.0), (1.0, n, 1.0), (1.0, n + 7, 2.0), (1.0, 0, 0.0), (1.0, 0, -1.0), (1.0, 0, float("nan")),
            (1.0, 2 ** 31 - 1, 1.0), (float("inf"), 0, 1.0), (1e-30, 0, 1.0), (1e30, 3, 0.5)]
    R = len(rows)
    xd = x.expand(R, n).contiguous().to(DEV)
    T, k, p = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    seed, pos = list(range(R)), [2 ** 40 + r for r in range(R)]
    tok, post, kept = _op(xd, T, k, p, seed, pos)
    assert post == [c + 1 for c in pos]
    stats = [0, 0]
    _check_rows(x.expand(R, n), tok, kept, T, k, p, seed, pos, stats)
    assert stats[1] == 0 and kept[:7] == [n] * 7 and kept[8] == n
    assert tok[8] == int(x[0].float().argmax())                        # T -> 0: all the mass on the maximum
