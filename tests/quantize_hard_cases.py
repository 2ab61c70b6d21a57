"""Inputs, models and checkers for the quantiser's hard cases (host: tests/test_quantize_hard_cases_host.py, GPU:
tests/test_gpu_quantize_hard_cases.py): exact ties, deep holes, points far outside the ball and panels that saturate.  CPU only.

Why equality can be asserted.  Every coordinate of the 65 536 E8P12 codewords is a multiple of 1/4 in [0.25, 2.75] in absolute
value, squared norms are at most 16.5, and two codewords are at squared distance >= 2 (inradius 0.7071).  The abs-table entries
b are multiples of 1/2, at most 3.5.  For a target x on the grid 2^-g with |x_j| <= X, every number e8p_scan (csrc/quantize.hip)
forms -- y = x -+ 1/4, the products b_j |y_j|, their running sum, 2 s sum(x), the score -- is a multiple of 2^-(max(g, 2) + 1)
of magnitude at most S = 56 (X + 1/4) + 4 X + 17, so all of it is exact in fp32 when S 2^(max(g, 2) + 1) <= 2^24
(`scan_is_exact`): 2^14 for multiples of 1/8 up to 16.  No rounding takes part, fused or not; the kernel must return an exactly
nearest codeword, and exactly the one its documented tie rule names."""
import numpy as np
import torch

from oracle import quip_oracle as O

from tests import ldlq_cases as C
from tests import ldlq_rvq_cases as R

U32 = C.U32
SIGMA_REG = 0.01                      # quip.py's default regulariser
_GRID = O.e8p_full_grid_f64()
_GRID_N2 = (_GRID * _GRID).sum(-1)


# ---- exactness premise -------------------------------------------------------------------------------------------------------

def grid_bits(X, limit=8):
    """smallest g <= limit with X 2^g integral, or None"""
    X = np.asarray(X, np.float64)
    if not np.isfinite(X).all():
        return None
    for g in range(limit + 1):
        if np.array_equal(np.round(X * 2.0 ** g), X * 2.0 ** g):
            return g
    return None


def scan_is_exact(X):
    """the premise of the module docstring for every row of X (N, 8)"""
    g = grid_bits(X)
    if g is None:
        return False
    mx = float(np.abs(X).max()) if np.size(X) else 0.0
    return (56.0 * (mx + 0.25) + 4.0 * mx + 17.0) * 2.0 ** (max(g, 2) + 1) <= 2.0 ** 24


# ---- the float64 brute force, with its ties ----------------------------------------------------------------------------------

def _score_chunks(X, grid, chunk):
    X = np.asarray(X, np.float64)
    gn = _GRID_N2 if grid is _GRID else (grid * grid).sum(-1)
    for i in range(0, X.shape[0], chunk):
        yield i, 2.0 * X[i:i + chunk] @ grid.T - gn


def exact_winners(X, grid=None, chunk=256):
    """bool (N, codes): the codes whose float64 score 2 x.g - |g|^2 equals the row's maximum.  grid: the full E8P12 grid
    (default) or any (codes, 8) table such as O.e81b_grid().  On exact inputs the scores carry no rounding, so this is the set
    of nearest codewords."""
    grid = _GRID if grid is None else np.asarray(grid, np.float64)
    out = np.zeros((np.asarray(X).shape[0], grid.shape[0]), dtype=bool)
    for i, S in _score_chunks(X, grid, chunk):
        out[i:i + S.shape[0]] = S == S.max(axis=1, keepdims=True)
    return out


class WinnerStats:
    """of exact_winners without keeping the (N, 65 536) array: count per row, the lowest winning code, the maximal score, and
    whether codes[i] is a winner of row i.  Equal (row, code) pairs are scored once."""
    def __init__(self, X, codes=None, grid=None, chunk=256):
        grid = _GRID if grid is None else np.asarray(grid, np.float64)
        X = np.asarray(X, np.float64)
        key = X if codes is None else np.concatenate([X, np.asarray(codes, np.float64)[:, None]], axis=1)
        if np.isnan(key).any():
            uniq, inv = key, np.arange(key.shape[0])
        else:
            uniq, inv = np.unique(key, axis=0, return_inverse=True)
            inv = inv.reshape(-1)
        Xu = uniq[:, :8]
        cu = None if codes is None else uniq[:, 8].astype(np.int64)
        n = Xu.shape[0]
        count, lowest, best = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.float64)
        contains = None if codes is None else np.zeros(n, bool)
        for i, S in _score_chunks(Xu, grid, chunk):
            sl = slice(i, i + S.shape[0])
            best[sl] = S.max(axis=1)
            win = S == best[sl, None]
            count[sl] = win.sum(axis=1)
            lowest[sl] = win.argmax(axis=1)
            if codes is not None:
                contains[sl] = win[np.arange(S.shape[0]), cu[sl]]
        self.count, self.lowest, self.best = count[inv], lowest[inv], best[inv]
        self.contains = None if codes is None else contains[inv]


def score64(X, codes, grid=None):
    grid = _GRID if grid is None else np.asarray(grid, np.float64)
    g = grid[np.asarray(codes)]
    return 2.0 * (np.asarray(X, np.float64) * g).sum(-1) - (g * g).sum(-1)


def decode_e8p(codes):
    """fp32 codewords of E8P12 codes, shape codes.shape + (8,)"""
    return O.e8p_decode_i8(np.asarray(codes).astype(np.uint16)).astype(np.float32) / np.float32(4)


# ---- the documented tie rule ----------------------------------------------------------------------------------------------------

def _abs_table():
    """signed abs-table rows b_e (256, 8) in natural column order, from the packed table: column p is byte
    O.E8P_BYTE_OF_POS[p] over 4; column 7 is negative where the row's sum is odd"""
    by = np.ascontiguousarray(O.e8p_grid_packed_abs()).view(np.int8).reshape(256, 8)
    return by[:, list(O.E8P_BYTE_OF_POS)].astype(np.float64) / 4.0


def tie_rule_code(X, chunk=512, last_cheapest=False):
    """The rule of csrc/quantize.hip's header as numpy in float64, one candidate codeword per (e, par):
        s = +1/4 (par 0) or -1/4 (par 1), y = x - s; g_j - s takes the sign of y_j, y_j == 0 counting as positive, and the
        magnitude |b_ej|; that is g = D b_e + s with D_j = sign(y_j) sign(b_ej).  If D holds an odd number of -1, the column
        with the smallest |b_ej| |y_j| is flipped, the lowest-index one among equals.
    The winner is the candidate with the largest 2 x.g - |g|^2; among equals the lowest e, then par 0 before par 1.
    code = e << 8 | (sv ^ par), bit 7 - [0, 2, 1, 3, 4, 6, 5, 7][j] of sv set where D_j = -1.
    last_cheapest=True is the planted fault of the host test: the LAST cheapest column is flipped instead."""
    X = np.asarray(X, np.float64)
    b = _abs_table()
    absb, bsign = np.abs(b), np.where(b < 0, -1.0, 1.0)
    bitpos = np.array([7 - O.E8P_BYTE_OF_POS[j] for j in range(8)])
    out = np.zeros(X.shape[0], np.int64)
    for i in range(0, X.shape[0], chunk):
        x = X[i:i + chunk]
        n = x.shape[0]
        scores = np.empty((n, 256, 2))
        svs = np.empty((n, 256, 2), np.int64)
        for par, s in ((0, 0.25), (1, -0.25)):
            y = x - s
            sig = np.where(y < 0, -1.0, 1.0)[:, None, :]                        # (n, 1, 8): sign of g_j - s
            D = sig * bsign[None]                                               # (n, 256, 8)
            cost = absb[None] * np.abs(y)[:, None, :]
            odd = (D < 0).sum(-1) % 2 == 1
            if last_cheapest:
                jm = 7 - np.argmin(cost[..., ::-1], axis=-1)
            else:
                jm = np.argmin(cost, axis=-1)                                   # first minimum
            flip = odd[..., None] & (np.arange(8) == jm[..., None])
            D = np.where(flip, -D, D)
            g = D * b[None] + s
            scores[:, :, par] = 2.0 * (x[:, None, :] * g).sum(-1) - (g * g).sum(-1)
            svs[:, :, par] = ((D < 0) << bitpos).sum(-1)
        key = scores.reshape(n, 512).argmax(axis=1)                             # first maximum in (e, par) order
        e, par = key >> 1, key & 1
        out[i:i + n] = (e << 8) | (svs[np.arange(n), e, par] ^ par)
    return out


def lowest_index_code(X, grid):
    """the documented rule of the 256-entry E81B scan: the lowest index among the maximal float64 scores"""
    grid = np.asarray(grid, np.float64)
    return (2.0 * np.asarray(X, np.float64) @ grid.T - (grid * grid).sum(-1)).argmax(axis=1)


# ---- the score bound of the tolerance groups -----------------------------------------------------------------------------------

def score_bound(X):
    """First-order bound (u = 2^-24) on |fp32 score - exact score| of any candidate (e, par) in e8p_scan, per row of X, from
    counting the scan's operations:
      y_j = x_j - s                    one rounding, u |y_j|; through the product it costs u t_j, t_j = b_j |y_j|
      t_j = b_j |y_j|                  one rounding, u t_j (none when contracted into the sum)
      sum  = t_0 + ... + t_7           8 additions from 0, each at most u T, T = sum_j t_j
         => |d sum| <= 10 u T
      mn = min_j t_j                   a copy of one t_j: 2 u T at most;  2 mn exact
      sum - 2 mn                       one rounding, u T                  => inner error <= (10 + 4 + 1) u T = 15 u T
      2 (sum - 2 mn)                   exact                              => 30 u T
      sx = x_0 + ... + x_7             7 roundings, 7 u |x|_1
      cs = 2 s sx - 1/2                2 s sx exact (|2 s| = 1/2): 3.5 u |x|_1, the subtraction u (|x|_1 / 2 + 1/2)
         => |d cs| <= u (4 |x|_1 + 1/2)
      2 inner + cs                     one rounding, u (2 T + |x|_1 / 2 + 1/2)
      ... - n2                         one rounding, u (2 T + |x|_1 / 2 + 1/2 + 12)   (n2 = |b_e|^2 <= 12, exact)
    Sum: u (34 T + 5 |x|_1 + 13.5), with T <= max|b| (|x|_1 + 8/4).  The kernel's winner therefore has an exact score within
    2 bound of the maximum, i.e. ||x - g||^2 - ||x - g*||^2 <= 2 bound(x)."""
    l1 = np.abs(np.asarray(X, np.float64)).sum(-1)
    T = float(np.abs(_abs_table()).max()) * (l1 + 2.0)
    return U32 * (34.0 * T + 5.0 * l1 + 13.5)


def excess_over_nearest(X, codes):
    """||x - g||^2 - ||x - g*||^2 per row as a difference of float64 scores, g = the decoded codes, g* the brute-force nearest"""
    _, star = O.round_dense(X, _GRID)
    return score64(X, star) - score64(X, codes)


# ---- search inputs -------------------------------------------------------------------------------------------------------------

def _neighbours(code):
    """codes at squared distance 2 of `code`, split by kind: same abs row | another abs row, same shift | the other shift"""
    d2 = ((_GRID - _GRID[code]) ** 2).sum(-1)
    nb = np.nonzero(d2 == 2.0)[0]
    par = lambda c: np.asarray(O._popcount8(np.asarray(c) & 0xff)) & 1      # noqa: E731
    same_row = (nb >> 8) == (code >> 8)
    same_shift = par(nb) == par(np.array([code]))[0]
    return nb[same_row], nb[~same_row & same_shift], nb[~same_shift]


def _midpoints(rng, n_codes=120, per_kind=2):
    rows, kinds = [], []
    for a in rng.choice(65536, n_codes, replace=False):
        for kind, nb in enumerate(_neighbours(int(a))):
            for bcode in rng.permutation(nb)[:per_kind]:
                rows.append((_GRID[a] + _GRID[bcode]) / 2.0)
                kinds.append(kind)
    return np.asarray(rows), np.asarray(kinds)


def _repair_ties(rng, n=512):
    """x = s + y with |y_j| = |b_ej| (the lattice coordinate) except two or more columns of equal b shrunk to one small value v,
    b v below every other b_j |y_j|, and an odd number of sign flips relative to b_e: candidate (e, par) must repair, and its
    cheapest column is not unique"""
    b = _abs_table()
    rows = [np.where(np.arange(8) % 2 == 0, -0.5, 0.5) * np.array([1, 1, 1, 1, 1, 1, 1, -1.0]) + 0.25]   # all |y_j| equal
    while len(rows) < n:
        e, par = int(rng.integers(256)), int(rng.integers(2))
        ab = np.abs(b[e])
        val = 0.5                    # only columns of 1/2 are shrunk: no abs row has a smaller entry to offer there
        cols = np.nonzero(ab == val)[0]
        if len(cols) < 2:
            continue
        cols = rng.choice(cols, int(rng.integers(2, len(cols) + 1)), replace=False)
        vs = [v for v in (0.0, 0.125, 0.25, 0.375) if val * v < 0.25]           # below b_j^2 >= 1/4 of every other column
        if not vs:
            continue
        v = rng.choice(vs)
        mag = ab.copy()
        mag[cols] = v
        sig = np.where(b[e] < 0, -1.0, 1.0)                                     # D = +1 everywhere
        flips = rng.choice(8, int(rng.choice([1, 3, 5])), replace=False)        # an odd number of -1
        sig[flips] *= -1.0
        y = sig * mag
        y[(mag == 0)] = 0.0                                                     # +0: counts as positive
        if ((np.where(y < 0, -1.0, 1.0) * np.where(b[e] < 0, -1.0, 1.0)) < 0).sum() % 2 == 0:
            continue                                                            # a zeroed column took the odd flip away
        rows.append(y + (0.25 if par == 0 else -0.25))
    rows = np.asarray(rows)
    # the repair tie of candidate (e, par) is a tie of the search only where that candidate wins: keep the rows with two or
    # more nearest codewords (decided by the float64 brute force alone; 504 of 512 at seed 0)
    return rows[WinnerStats(rows).count >= 2]


_SEARCH = None
EXACT_GROUPS = ("planes", "midpoints", "holes", "repair_ties", "dyadic8", "dyadic4", "dyadic2", "outside")
TOLERANCE_GROUPS = ("huge", "tiny", "nonfinite")
TIE_GROUPS = ("midpoints", "holes", "repair_ties")       # every row has at least two exact winners
MIDPOINT_KINDS = None                                    # per row of "midpoints": 0 same abs row, 1 another row, 2 other shift


def search_cases():
    """{name: (N, 8) fp32}: EXACT_GROUPS (dyadic: on the 1/8, 1/4 and 1/2 grids) and TOLERANCE_GROUPS; seeded, built once"""
    global _SEARCH, MIDPOINT_KINDS
    if _SEARCH is not None:
        return _SEARCH
    rng = np.random.default_rng(0)
    one, eye = np.ones((1, 8)), np.eye(8)
    cases = {}
    mixed = rng.integers(-16, 17, (256, 8)) / 8.0
    hit = rng.random((256, 8)) < 0.4
    hit[np.arange(256), rng.integers(0, 8, 256)] = True
    mixed[hit] = rng.choice([-0.25, 0.25], int(hit.sum()))
    cases["planes"] = np.concatenate([0 * one, 0.25 * one, -0.25 * one, 0.5 * one, -0.5 * one, eye, -eye, mixed])
    cases["midpoints"], MIDPOINT_KINDS = _midpoints(rng)
    # holes: a +- e_i around codewords well inside the ball, so that the hole's other neighbours are codewords too
    inner = np.nonzero(_GRID_N2 <= 4.5)[0]
    a = _GRID[rng.choice(inner, 48, replace=False)]
    cases["holes"] = np.concatenate([(a[:, None, :] + eye[None]).reshape(-1, 8), (a[:, None, :] - eye[None]).reshape(-1, 8)])
    cases["repair_ties"] = _repair_ties(rng)
    cases["dyadic8"] = rng.integers(-24, 25, (1024, 8)) / 8.0
    cases["dyadic4"] = rng.integers(-6, 7, (512, 8)) / 4.0
    cases["dyadic2"] = rng.integers(-6, 7, (512, 8)) / 2.0
    far = _GRID[np.argsort(-_GRID_N2, kind="stable")[:64]]
    cases["outside"] = np.concatenate([far * 1.25, far * 2.0, far * 4.0, 16.0 * eye, -16.0 * eye, 4.0 * one, -4.0 * one])
    for name in EXACT_GROUPS:
        X = cases[name]
        # multiples of 1/8 up to 16; the one exception are the codewords x 1.25 of `outside` (odd multiples of 5/16), which
        # lie on the 1/16 grid, where the premise of the module docstring holds as well
        assert grid_bits(X) <= (4 if name == "outside" else 3) and np.abs(X).max() <= 16.0 and scan_is_exact(X), name
        assert np.array_equal(X.astype(np.float32).astype(np.float64), X)
    assert grid_bits(np.delete(cases["outside"], np.s_[:64], axis=0)) <= 3
    g = rng.standard_normal((3, 128, 8))
    cases["huge"] = np.concatenate([g[0] * 1e2, g[1] * 1e4, g[2] * 1e6])
    sub = np.float64(np.float32(1.401298464324817e-45))                         # the smallest fp32 subnormal
    tiny = rng.choice([-1.0, 1.0], (96, 8))
    tiny[:32] *= 1e-30
    tiny[32:64] *= sub * rng.integers(1, 1 << 22, (32, 8))
    tiny[64:] *= sub
    tiny[64:, ::2] = 0.0
    cases["tiny"] = tiny
    nf = rng.standard_normal((64, 8))
    nf[0::8, 3] = np.nan
    nf[1::8] = np.nan
    nf[2::8, 0] = np.inf
    nf[3::8, 7] = -np.inf
    nf[4::8, 5] = 3e38
    nf[5::8] = -3e38
    nf[6] = np.inf
    cases["nonfinite"] = nf
    _SEARCH = {k: np.ascontiguousarray(v.astype(np.float32)) for k, v in cases.items()}
    return _SEARCH


def nonfinite_rows(X):
    X = np.asarray(X)
    return ~np.isfinite(X).all(axis=1) | (np.abs(X) >= 1e38).any(axis=1)


_STATS = {}


def search_reference(name):
    """(WinnerStats, tie_rule_code) of an exact group, computed once and shared"""
    if name not in _STATS:
        X = search_cases()[name]
        rule = tie_rule_code(X)
        _STATS[name] = (WinnerStats(X, rule), rule)
    return _STATS[name]


def check_search(X, vals, idx, stats, rule):
    """the three equalities of the exact groups -> (rows whose vals are not the decode of idx, rows whose idx is no exact
    winner, rows whose idx is not the tie rule's); stats = WinnerStats(X, idx)"""
    idx = np.asarray(idx)
    return (int((np.asarray(vals) != decode_e8p(idx)).any(axis=1).sum()), int((~stats.contains).sum()),
            int((idx != rule).sum()))


# ---- panel inputs -------------------------------------------------------------------------------------------------------------

PANEL_M = (1, 31, 32, 33, 65)
PANEL_C = (8, 16, 120, 128)
EXACT_SCALES = (-1.0, 0.25)
ILL_SHAPES = ((40, 384), (33, 688))


def signed_permutations(rng, groups):
    P = np.zeros((groups, 8, 8), np.float32)
    for k in range(groups):
        P[k, np.arange(8), rng.permutation(8)] = rng.choice([-1.0, 1.0], 8)
    return P


def integer_feedback(m, c, with_p, seed=0):
    """(A, B, M, P) fp32 numpy: A, B multiples of 1/8 in [-3, 3]; M entries in {0, +-1}, strictly lower block triangular in
    effect (rows j of groups right of column k's group), at most two non-zeros per column and source group; P None or signed
    8 x 8 permutations.  hat is a multiple of 1/4 (1/16 with the residual at scale 1/4), so E and every target stay dyadic:
    |E| <= 3 + 2 * 3.75 and |t| <= 6 + 30 * 10.5 < 2^9."""
    rng = np.random.default_rng(7919 * m + 31 * c + seed + (1 if with_p else 0))
    A = rng.integers(-24, 25, (m, c)) / 8.0
    B = rng.integers(-24, 25, (m, c)) / 8.0
    M = np.zeros((c, c))
    for col in range(c):
        for src in range(col // 8 + 1, c // 8):
            rows = rng.choice(8, int(rng.integers(0, 3)), replace=False)
            M[8 * src + rows, col] = rng.choice([-1.0, 1.0], len(rows))
    P = signed_permutations(rng, c // 8) if with_p else None
    return A.astype(np.float32), B.astype(np.float32), M.astype(np.float32), P


def zero_case(m, c, with_p):
    """A = B = 0 and no coupling: every group of every row is the tie at the origin (through P when given)"""
    A, B, M, P = integer_feedback(m, c, with_p)
    return np.zeros_like(A), np.zeros_like(B), np.zeros_like(M), P


def ill_conditioned_H(n, seed=0):
    """pairs of features equal up to 1e-3 noise, fewer samples than features, mean diagonal 1, plus SIGMA_REG I"""
    rng = np.random.default_rng(n + seed)
    samples = n // 2
    half = rng.standard_normal((samples, n // 2))
    X = np.repeat(half, 2, axis=1)[:, :n] + 1e-3 * rng.standard_normal((samples, n))
    H = X.T @ X / samples
    return (H / np.diag(H).mean() + SIGMA_REG * np.eye(n)).astype(np.float32)


def ill_conditioned(m, n):
    W, _ = C.make_case(m, n)
    return W, ill_conditioned_H(n)


def saturating(m, n):
    W, H = C.make_case(m, n)
    W = W.copy()
    W[0::5] *= 8.0
    W[2::11] *= 100.0
    W[:, n // 3] *= 50.0
    return W, H


def stage2_allowed(cbid, s):
    """second-stage codes b with ||b|| |s| < 0.70, inside the inradius 0.7071 of the first stage"""
    g = R.stage2_grid(cbid)
    return np.nonzero(np.sqrt((g * g).sum(-1)) * abs(float(np.float32(s))) < 0.70)[0]


def fixed_point(cbid, m, n, s=None, seed=0):
    """(W fp32 (m, n), planted codes int64 (m, n / 8)): W made of codewords -- E8P12 rows, or fl32(a + fl32(b s32)) with b
    from stage2_allowed.  a is then the only codeword within the inradius of W, the residual fl32(fl32(W - a) / s32) is b up
    to an fp32 rounding of W over |s| (far inside E8P12's and E81B's own inradii), and hat == W, so whatever H, the feedback is
    identically zero."""
    rng = np.random.default_rng(100 * m + n + seed)
    ca = rng.integers(0, 65536, (m, n // 8))
    a = decode_e8p(ca)
    if cbid == "E8P12":
        return a.reshape(m, n), ca
    s = R.DEFAULT_SCALE[cbid] if s is None else s
    cb_ = rng.choice(stage2_allowed(cbid, s), (m, n // 8))
    b = R.stage2_grid(cbid)[cb_].astype(np.float32)
    W = (a + (b * np.float32(s)).astype(np.float32)).astype(np.float32)
    return W.reshape(m, n), (ca << R.CODE_SHIFT[cbid]) | cb_


def poisoned(m, c, seed=0):
    """(A, B, M, P, bad rows): ordinary operands as in the existing panel tests, with one row all NaN (the LAST row: lanes past
    the end of the last workgroup replicate it), one holding +inf and one holding 3e38"""
    g = torch.Generator().manual_seed(100 * c + m + seed)
    A = torch.randn(m, c, generator=g) * 1.1
    B = torch.randn(m, c, generator=g) * 0.2
    M = torch.randn(c, c, generator=g) * 0.1
    P = (torch.eye(8) + 0.1 * torch.randn(c // 8, 8, 8, generator=g)).contiguous()
    bad = [m - 1, 2, 5]
    A[m - 1] = float("nan")
    A[2, c // 2] = float("inf")
    B[5, c - 1] = 3e38
    return A.numpy(), B.numpy(), M.numpy(), P.numpy(), bad


# ---- host models of the panels with the documented rules as the searches ----------------------------------------------------------

def rule_quantize(X):
    """(vals, idx) of the E8P12 step with tie_rule_code as the search, for ldlq_cases.panel_model"""
    idx = tie_rule_code(np.asarray(X, np.float64))
    return _GRID[idx], idx


class RuleCodebook:
    """what panel_model_rvq reads of a residual codebook: the classes' arithmetic in X's dtype with tie_rule_code as the E8P12
    search and the lowest-index arg max for E81B"""
    def __init__(self, cbid, s):
        self.id, self.opt_resid_scale = cbid, s

    def _e8p(self, X):
        idx = tie_rule_code(X.numpy().astype(np.float64))
        return torch.from_numpy(_GRID[idx]).to(X.dtype), torch.from_numpy(idx)

    def quantize(self, X, return_idx=True):
        a, ca = self._e8p(X)
        r = (X - a) / self.opt_resid_scale
        if self.id == "E8P12RVQ4B":
            b, cb_ = self._e8p(r)
        else:
            g = O.e81b_grid()
            cb_ = torch.from_numpy(lowest_index_code(r.numpy(), g))
            b = torch.from_numpy(g[cb_.numpy()]).to(X.dtype)
        final = a + b * self.opt_resid_scale
        return (final, (ca << R.CODE_SHIFT[self.id]) + cb_) if return_idx else final


def run_model(step, A, B, M, P, s=None):
    """(hat fp32, idx int64) numpy of the host model of `step` ("E8P12" or a residual codebook) on numpy operands, in float64
    (exact on the exact cases)"""
    t = lambda a: None if a is None else torch.from_numpy(np.asarray(a, np.float64))      # noqa: E731
    if step == "E8P12":
        hat, idx = C.panel_model(t(A), t(B), t(M), t(P), quantize=rule_quantize)
    else:
        hat, idx = R.panel_model_rvq(RuleCodebook(step, s))(t(A), t(B), t(M), t(P))
    return hat.numpy().astype(np.float32), idx.numpy()


# ---- the exact step checker ------------------------------------------------------------------------------------------------------

class ExactReport:
    def __init__(self):
        self.steps = self.premise = self.decode = self.winner = self.rule = self.winner2 = self.rule2 = 0

    @property
    def failures(self):
        return self.premise + self.decode + self.winner + self.rule + self.winner2 + self.rule2

    def __str__(self):
        return (f"{self.steps} steps: {self.premise} outside the premise, {self.decode} hat != decode(idx), {self.winner} / "
                f"{self.winner2} no exact winner (stage 1 / 2), {self.rule} / {self.rule2} not the tie rule's code")


def check_exact_steps(A, B, M, P, hat, idx, step, s=None):
    """Every group of every row of one ldlq_panel / ldlq_panel_rvq call on exact operands.  The target is recomputed in
    float64 from the operands and the GIVEN hat right of the group,
        t_k = A_k + (B_k + sum_{j > k} (A_j - hat_j) M[j, k]) P_k,
    and the following are counted per step (all must be 0):
      premise   t_k not dyadic (a multiple of 2^-4), |t| >= 2^20, or outside scan_is_exact (for the residual r as well)
      decode    hat_k is not the fp32 decode of idx_k: the codeword, or fl32(a + fl32(b s)) of the two stage codes
      winner    the first-stage code is not in exact_winners(t_k);        winner2: the same for the second stage on
      rule      it is not tie_rule_code(t_k);                             rule2:   r = (t_k - a) / s (exact: s = -1 or 1/4),
                                                                          for E81B with the lowest index as the rule
    step: "E8P12", "E8P12RVQ4B" or "E8P12RVQ3B".  -> ExactReport"""
    A, B, M = (np.asarray(a, np.float64) for a in (A, B, M))
    hat32, idx = np.asarray(hat, np.float32), np.asarray(idx).astype(np.int64)
    m, c = A.shape
    E = A - hat32.astype(np.float64)
    rep = ExactReport()
    T = np.empty((c // 8, m, 8))
    for k in range(c // 8):
        lo, hi = 8 * k, 8 * k + 8
        t = B[:, lo:hi] + E[:, hi:] @ M[hi:, lo:hi]
        if P is not None:
            t = t @ np.asarray(P[k], np.float64)
        T[k] = A[:, lo:hi] + t
    flat = T.reshape(-1, 8)
    codes = idx.T.reshape(-1)                                                   # the same (k, row) order
    hat_k = hat32.reshape(m, c // 8, 8).transpose(1, 0, 2).reshape(-1, 8)
    rep.steps = flat.shape[0]
    g = grid_bits(flat)
    rep.premise = int(g is None or g > 4 or np.abs(flat).max() >= 2.0 ** 20 or not scan_is_exact(flat))
    if step == "E8P12":
        ca = codes
        rep.decode = int((hat_k != decode_e8p(ca)).any(axis=1).sum())
    else:
        ca, cb_ = R.split_codes(step, codes)
        rep.decode = int((hat_k != R.decode_f32(step, codes, s)).any(axis=1).sum())
    rep.winner = int((~WinnerStats(flat, ca).contains).sum())
    rep.rule = int((ca != tie_rule_code(flat)).sum())
    if step != "E8P12":
        r = (flat - _GRID[ca]) / float(s)
        if step == "E8P12RVQ4B":
            rep.premise += int(not scan_is_exact(r))
            rep.winner2 = int((~WinnerStats(r, cb_).contains).sum())
            rep.rule2 = int((cb_ != tie_rule_code(r)).sum())
        else:
            g2 = O.e81b_grid()
            gb = grid_bits(r)
            # E81B entries are multiples of 1/2 up to 2: products and sums on the grid 2^-(gb + 1), below 8 * 2 * max|r| + 2
            rep.premise += int(gb is None or (32.0 * np.abs(r).max() + 2.0) * 2.0 ** (gb + 1) > 2.0 ** 24)
            rep.winner2 = int((~WinnerStats(r, cb_, grid=g2).contains).sum())
            rep.rule2 = int((cb_ != lowest_index_code(r, g2)).sum())
    return rep
