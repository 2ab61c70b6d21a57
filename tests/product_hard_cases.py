"""Inputs that drive the quantised products to the ends of their stated ranges instead of the sqrt(K) middle that randn
and random codes reach, and a model of the integer-domain product, for the host checks
(tests/test_product_hard_cases_host.py) and the launches (tests/test_gpu_product_hard_cases.py).  CPU only.

Codes aligned to a sign vector.  Given t in {+-1}^k, every group of a row holds the code that maximises t_g . w (or
-t_g . w: anti-aligned); row r of an (n, k) layer is aligned on its first a_r groups and anti-aligned on the rest,
a_r = linspace(0, k / group, n).  With x = t * magnitude one layer ramps from -sum|x w| through rows that cancel to
about 0 up to +sum|x w|.

    E8P12        arg max over oracle.e8p_full_grid_i8(), one table entry per 8-bit sign pattern
    D4           arg max over oracle.d4_grid(), per 4-sign pattern
    HI           nibble 15 (w = +7.5) or 0 (w = -7.5)
    E8P12RVQ4B   main code aligned; residual code aligned when the residual scale is positive, anti-aligned when it is
    E8P12RVQ3B   negative (RVQ3: the residual is an E81B row, arg max over oracle.e81b_grid())

What the matrix-core GEMV multiplies is the VIRTUAL pair of DESIGN 4.2: for E8P12 and D4 the row and x themselves, for
the RVQ codebooks the 2k-wide row whose 8-groups alternate residual / main codes against x' = [s x_g | x_g]_g, for HI
the 2k-wide D4-style row against x' = [x0 x2 0 0 | x4 x6 0 0 | x1 x3 0 0 | x5 x7 0 0]_g.  Layer.W_int holds the
virtual row as the integers the tables hold (4w: log2_unit 2; D4 / HI 2w: log2_unit 1), virtual_x() the fp16 vector.

Activation kinds, x = t * magnitude in fp16 (KINDS):

    flat       every |x| = c, c a power of two
    flat_top   every |x| = (2 - 2^-10) c: X = 2^22 - 2^11, digit h = 64, m = -8
    tiers      |x| = c, c 2^-8, c 2^-16 by index mod 3: each digit plane carries an aligned sum of its own
    top_mix    |x| = (2 - 2^-10) c and (63 / 32) c in turn (h = 64 and 63), element 0 at 63 / 32 as well: an odd number
               of odd terms, so the top-of-range sums are odd (beyond 2^24 not fp32 values, see product_model)
    outlier    |randn| with one element 3000 (times c)
    onehot     a single c at a chosen column
    subnormal  every |x| = 2^-24
    overflow   flat at 4 c: the outer rows overflow fp16, the middle rows do not

c is the largest power of two (up to 2^15, the largest fp16 holds) with c * max_r sum_i m_i |w_ri| < 65504 (m the kind's
magnitudes at c = 1, w the virtual row), so that no row of any kind but `overflow` can leave fp16.

The model (planes_of_fp16, product_model) restates DESIGN 4.2 and nothing of the kernels."""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import quip_oracle as O

KINDS = ("flat", "flat_top", "tiers", "top_mix", "outlier", "onehot", "subnormal", "overflow")
EXACT_KINDS = ("flat", "flat_top", "tiers", "overflow")     # block fixed point holds every element exactly
CODEBOOKS = (("E8P12", None), ("D4", None), ("HI", None), ("E8P12RVQ4B", 1 / 3.45), ("E8P12RVQ4B", -1.0),
             ("E8P12RVQ3B", 1 / 2.04))
GROUP = {"E8P12": 8, "D4": 4, "HI": 8, "E8P12RVQ4B": 8, "E8P12RVQ3B": 8}
ONEHOT_COLS = (0, 7, 8, 511, 512, -1)
# k at which the GPU tests run, every codebook (one slice; Kp padding next to saturated digits; one-shot; phases /
# streaming / K split).  The 2k-wide virtual rows of HI and the RVQ codebooks are 57344 long at k = 28672: the op's
# dispatcher sends them to the K-splitting kernel (its D4 table mode for HI, its third table for RVQ3B); RVQ3B's
# 14336 is the shortest of its virtual rows (beyond 25600) that takes that route.
_KS = (512, 1152, 4096, 11008, 28672)
SHAPES = {"E8P12": _KS, "D4": _KS, "HI": _KS, "E8P12RVQ4B": _KS, "E8P12RVQ3B": _KS[:4] + (14336, 28672)}
NS = (37, 257)
V2_DYNAMIC = (2048, 14336)      # (n, k) at which the K-splitting kernel's waves pull runs from the counter


# ----------------------------------------------------------------------------------------------------------------
# aligned codes
# ----------------------------------------------------------------------------------------------------------------

def sign_patterns(width):
    """(2^width, width) of +-1: bit p of the pattern index set <=> t_p = -1"""
    return (1 - 2 * ((np.arange(1 << width)[:, None] >> np.arange(width)) & 1)).astype(np.float64)


def pattern_of(t, width):
    """(k,) +-1 -> (k / width,) pattern indices"""
    neg = (np.asarray(t).reshape(-1, width) < 0).astype(np.int64)
    return (neg << np.arange(width)).sum(1)


@functools.lru_cache(maxsize=None)
def aligned_table(name):
    """(winner index, its score) per sign pattern for the grid `name`: e8p (scores in units of 4w), d4, e81b (in w)"""
    grid = {"e8p": lambda: O.e8p_full_grid_i8().astype(np.float64), "d4": O.d4_grid, "e81b": O.e81b_grid}[name]()
    scores = sign_patterns(grid.shape[1]) @ np.asarray(grid, dtype=np.float64).T    # small integers / halves: exact
    return scores.argmax(1), scores.max(1)


def sign_vector(k, seed):
    return np.random.default_rng(seed).choice([-1.0, 1.0], k)


def row_split(n, groups):
    """a_r: row r is aligned on its first a_r groups"""
    return np.rint(np.linspace(0, groups, n)).astype(np.int64)


def fp16_scale(scale):
    return None if scale is None else float(np.float16(scale))


def aligned_codes(cbid, t, n, scale=None):
    """Qidxs (n, cols) as the codebook stores them"""
    k = len(t)
    g = GROUP[cbid]
    groups = k // g
    al = np.arange(groups)[None, :] < row_split(n, groups)[:, None]          # (n, groups): aligned here?
    if cbid == "HI":
        idx = np.where(np.repeat(al, g, axis=1) == (np.asarray(t) > 0)[None, :], 15, 0)
        return O.hi_pack(idx)
    if cbid == "D4":
        lut, _ = aligned_table("d4")
        pat = pattern_of(t, 4)
        return np.where(al, lut[pat][None, :], lut[pat ^ 15][None, :]).astype(np.uint8)
    lut, _ = aligned_table("e8p")
    pat = pattern_of(t, 8)
    main = np.where(al, lut[pat][None, :], lut[pat ^ 255][None, :]).astype(np.int64)
    if cbid == "E8P12":
        return main.astype(np.uint16).view(np.int16)
    rpat = pat if scale > 0 else pat ^ 255               # s * resid along t: resid along sign(s) t
    if cbid == "E8P12RVQ4B":
        res = np.where(al, lut[rpat][None, :], lut[rpat ^ 255][None, :]).astype(np.int64)
        return ((main << 16) | res).astype(np.uint32).view(np.int32)
    assert cbid == "E8P12RVQ3B" and k % 32 == 0
    lut3, _ = aligned_table("e81b")
    res = np.where(al, lut3[rpat][None, :], lut3[rpat ^ 255][None, :]).astype(np.int64)
    return O.rvq3_pack(((main << 8) | res).astype(np.int32))


def int_weights(cbid, Qidxs):
    """the virtual row of DESIGN 4.2 as the integers the decode tables hold -> ((n, kv), log2_unit); the integers are
    kept in float64 (exact), the type product_model() sums them in"""
    W, unit = _int_weights(cbid, Qidxs)
    return W.astype(np.float64), unit


def _int_weights(cbid, Qidxs):
    n = Qidxs.shape[0]
    if cbid == "E8P12":
        return O.e8p_decode_i8(np.ascontiguousarray(Qidxs).view(np.uint16)).astype(np.int64).reshape(n, -1), 2
    if cbid == "D4":
        return np.rint(2 * O.d4_grid()[Qidxs.astype(np.intp)]).astype(np.int64).reshape(n, -1), 1
    if cbid == "HI":
        b = np.ascontiguousarray(Qidxs).view(np.uint8).astype(np.int64)                 # (n, k / 2) code bytes
        W = np.zeros(b.shape + (4,), np.int64)
        W[..., 0], W[..., 1] = 2 * (b & 15) - 15, 2 * (b >> 4) - 15
        return W.reshape(n, -1), 1
    if cbid == "E8P12RVQ4B":
        q = np.ascontiguousarray(Qidxs).view(np.uint32)
        main, res = (q >> 16).astype(np.uint16), (q & 0xFFFF).astype(np.uint16)
        rw = O.e8p_decode_i8(res).astype(np.int64)
    else:
        main, r8 = O.rvq3_split(Qidxs)
        rw = np.rint(4 * O.e81b_grid()[r8.astype(np.intp)]).astype(np.int64)
    mw = O.e8p_decode_i8(main).astype(np.int64)
    return np.concatenate([rw, mw], axis=-1).reshape(n, -1), 2                              # [resid 8 | main 8] per group


def virtual_x(cbid, x, scale=None):
    """the fp16 vector whose digit planes the product reads: x itself, [fp16(s x_g) | x_g]_g, or HI's spread"""
    x = np.asarray(x, dtype=np.float16)
    if cbid in ("E8P12", "D4"):
        return x
    g = x.reshape(-1, 8)
    if cbid == "HI":
        z = np.zeros((g.shape[0], 2), np.float16)
        return np.concatenate([g[:, [0, 2]], z, g[:, [4, 6]], z, g[:, [1, 3]], z, g[:, [5, 7]], z], axis=1).reshape(-1)
    s = np.float64(fp16_scale(scale))
    return np.concatenate([(s * g.astype(np.float64)).astype(np.float16), g], axis=1).reshape(-1)


class Layer(NamedTuple):
    cbid: str
    scale: Optional[float]      # opt_resid_scale of the RVQ codebooks
    n: int
    k: int
    t: np.ndarray               # (k,) +-1
    Qidxs: np.ndarray
    W_int: np.ndarray           # (n, kv) virtual row: integers held in float64
    log2_unit: int

    @property
    def W64(self):
        return self.W_int / (1 << self.log2_unit)

    @property
    def kv(self):
        return self.W_int.shape[1]


@functools.lru_cache(maxsize=8)
def make_aligned_layer(cbid, k, n, scale=None, seed=0):
    t = sign_vector(k, 1000 * seed + k)
    Q = aligned_codes(cbid, t, n, scale)
    W, unit = int_weights(cbid, Q)
    return Layer(cbid, scale, n, k, t, Q, W, unit)


# ----------------------------------------------------------------------------------------------------------------
# activations
# ----------------------------------------------------------------------------------------------------------------

def _unit_magnitude(kind, k, col, seed):
    if kind in ("flat", "overflow"):
        return np.ones(k)
    if kind == "flat_top":
        return np.full(k, 2.0 - 2.0 ** -10)
    if kind == "tiers":
        return 2.0 ** (-8.0 * (np.arange(k) % 3))
    if kind == "top_mix":
        return np.where((np.arange(k) % 2 == 0) & (np.arange(k) > 0), 2.0 - 2.0 ** -10, 63.0 / 32.0)
    if kind == "outlier":
        m = np.abs(np.random.default_rng(seed).standard_normal(k).astype(np.float16).astype(np.float64))
        m[(7 * k) // 16 + 3] = 3000.0
        return m
    if kind == "onehot":
        m = np.zeros(k)
        m[col] = 1.0
        return m
    raise KeyError(kind)


def activation(layer, kind, col=0, seed=0):
    """-> (x (k,) fp16, c).  c: the largest power of two that keeps every row of the virtual product inside fp16"""
    k = layer.k
    if kind == "subnormal":
        return (layer.t * 2.0 ** -24).astype(np.float16), 2.0 ** -24
    m = _unit_magnitude(kind, k, col % k, seed)
    mv = np.abs(virtual_x(layer.cbid, m.astype(np.float16), layer.scale).astype(np.float64))
    bound = float((np.abs(layer.W64) @ mv).max())
    c = 2.0 ** np.floor(np.log2(65504.0 / bound))
    if c * bound >= 65504.0:
        c /= 2
    c = min(c, 2.0 ** 15)                # (onehot at a column of small weights: x itself has to stay in fp16)
    if kind == "overflow":
        c *= 4
    x = (layer.t * m * c).astype(np.float16)
    # (outlier: a small |randn| times c < 1 may round in fp16's subnormals -- x is whatever fp16 holds)
    assert np.all(np.isfinite(x)) and (kind == "outlier" or np.array_equal(x.astype(np.float64), layer.t * m * c)), (kind, c)
    return x, c


# ----------------------------------------------------------------------------------------------------------------
# the model of the integer-domain product
# ----------------------------------------------------------------------------------------------------------------

def digits_of(X):
    """balanced int8 digits of X = h 65536 + m 256 + l (had::digits_of)"""
    X = np.asarray(X, dtype=np.int64)
    l = ((X & 0xFF) ^ 0x80) - 0x80
    X1 = (X - l) >> 8
    m = ((X1 & 0xFF) ^ 0x80) - 0x80
    h = (X1 - m) >> 8
    return h, m, l


def planes_of_fp16(x):
    """block fixed point of an fp16 vector: sh = 21 - E, E the exponent of the largest |x| (a subnormal counts as
    exponent -14), X = rint(x 2^sh) -> (h, m, l, sh)"""
    x = np.asarray(x, dtype=np.float16).reshape(-1)
    assert np.all(np.isfinite(x))
    ebits = int((x.view(np.uint16) & 0x7FFF).max()) >> 10
    sh = 21 - (max(ebits, 1) - 15)
    X = np.rint(x.astype(np.float64) * 2.0 ** sh).astype(np.int64)
    assert np.abs(X).max() < 2 ** 22
    h, m, l = digits_of(X)
    return h, m, l, sh


def product_model(h, m, l, sh, W_int, log2_unit):
    """exact integer sums S_d = sum_k digit_d[k] W_int[:, k]; f = fl32(S_h 65536 + fl32(S_m 256 + S_l)) (two fused
    multiply-adds, each rounding once); y = fp16(f 2^(-sh - log2_unit)), one rounding.  -> (y (n,) fp16, max |S_d|)

    The operands of a multiply-add are fp32 values, so each S_d enters as fl32(S_d).  Below 2^24 that is S_d itself and
    the statement above is the whole of it; beyond (the int32 range is 2^31) fl32(S_d) is S_d rounded to nearest even,
    one more rounding of at most 2^-25 of that sum -- the caller gets max |S_d| to know which case it is in."""
    Wf = np.asarray(W_int, dtype=np.float64)
    assert np.abs(Wf).sum(1).max() * 128 < 2.0 ** 53                                          # float64 sums are exact
    S = [np.rint(Wf @ np.asarray(d, dtype=np.float64)).astype(np.int64) for d in (h, m, l)]
    assert max(np.abs(Sd).max() for Sd in S) < 2 ** 31
    Sf = [Sd.astype(np.float32).astype(np.int64) for Sd in S]          # int64 -> fp32: round to nearest even
    inner = (Sf[1] * 256 + Sf[2]).astype(np.float32)                   # exact integer, then ONE rounding: the fma
    f = (Sf[0] * 65536 + inner.astype(np.int64)).astype(np.float32)     # inner is an integer below 2^63: exact addend
    with np.errstate(over="ignore"):
        y = (f.astype(np.float64) * 2.0 ** (-sh - log2_unit)).astype(np.float16)
    return y, int(max(np.abs(Sd).max() for Sd in S))


def model_of(layer, x):
    """the model on the planes the model itself makes of virtual_x(x) -> (y, max |S_d|, xv)"""
    xv = virtual_x(layer.cbid, x, layer.scale)
    h, m, l, sh = planes_of_fp16(xv)
    y, smax = product_model(h, m, l, sh, layer.W_int, layer.log2_unit)
    return y, smax, xv
