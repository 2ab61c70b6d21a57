"""tests/product_hard_cases.py on its own (no GPU): the builders keep their promises, the model of the integer-domain
product agrees with the float64 product (the "reference alone" condition of the GPU tests), and the integer sums stay in
range at every shape the GPU tests run."""
import numpy as np
import pytest

from oracle import quip_oracle as O
from tests import product_hard_cases as H
from tests.test_gpu_ops import _mm_tol

IDS = [f"{c}{'' if s is None else f'_{s:+.2f}'}" for c, s in H.CODEBOOKS]


def _group_scores(L):
    """(n, groups) of t'_g . w'_g over the real 8- (4-) groups: the virtual row against the sign of the virtual x"""
    tv = np.sign(H.virtual_x(L.cbid, L.t.astype(np.float16), L.scale).astype(np.float64))
    per = L.kv // (L.k // H.GROUP[L.cbid])
    return (L.W_int * tv[None, :]).reshape(L.n, -1, per).sum(-1), tv


@pytest.mark.parametrize("cbid,scale", H.CODEBOOKS, ids=IDS)
def test_aligned_groups_attain_the_brute_force_maximum(cbid, scale):
    """every aligned group holds a code that no other code beats along t_g, every anti-aligned one along -t_g; the
    brute force here goes over the grids per GROUP, not through the per-pattern tables of the builder"""
    k, n = 512, 37
    L = H.make_aligned_layer(cbid, k, n, scale)
    g = H.GROUP[cbid]
    tg = L.t.reshape(-1, g)
    if cbid == "HI":
        best = np.full(k // g, 15.0 * g)                                 # 2w = +-15 per element
    elif cbid == "D4":
        best = 2 * np.abs(O.d4_grid() @ tg.T).max(0)                     # the grid is symmetric: max over +-t
        assert np.array_equal(2 * (O.d4_grid() @ tg.T).max(0), best)
    else:
        e8 = O.e8p_full_grid_i8().astype(np.float64)
        best = (e8 @ tg.T).max(0)
        anti = (e8 @ (-tg).T).max(0)
        assert 32 <= best.min() and best.max() <= 42 and np.abs(e8).max() == 11
        if cbid != "E8P12":
            s = H.fp16_scale(scale)
            r = e8 if cbid == "E8P12RVQ4B" else 4 * O.e81b_grid()
            rbest, ranti = (r @ (np.sign(s) * tg).T).max(0), (r @ (-np.sign(s) * tg).T).max(0)
    score, tv = _group_scores(L)
    al = np.arange(k // g)[None, :] < H.row_split(n, k // g)[:, None]
    if cbid in ("HI", "D4"):
        want = np.where(al, best[None, :], -best[None, :])
    elif cbid == "E8P12":
        want = np.where(al, best[None, :], -anti[None, :])
    else:
        # virtual group = [resid | main] against [sign(s) t | t]: the two maxima add
        want = np.where(al, (best + rbest)[None, :], -(anti + ranti)[None, :])
    assert np.array_equal(score, want)
    assert al[0].sum() == 0 and al[-1].all() and 0 < al[n // 2].sum() < k // g


@pytest.mark.parametrize("cbid,scale", H.CODEBOOKS, ids=IDS)
def test_rows_ramp_from_minus_to_plus_the_absolute_sum(cbid, scale):
    """row 0 gives -sum|x w| and the last row +sum|x w| (every element of an aligned code has the sign of t), the rows
    between rise monotonically through a row that nearly cancels"""
    L = H.make_aligned_layer(cbid, 1152, 37, scale)
    x, c = H.activation(L, "flat")
    xv = H.virtual_x(cbid, x, scale).astype(np.float64)
    y = L.W64 @ xv
    absdot = np.abs(L.W64) @ np.abs(xv)
    if cbid == "E8P12RVQ3B":
        # E81B's half-integer roots have an even number of minus signs: the winner of a pattern with an odd number
        # carries one element (s / 2 of some 25 per group) against t -- the group maxima are the test above's
        assert -absdot[0] <= y[0] <= -0.97 * absdot[0] and 0.97 * absdot[-1] <= y[-1] <= absdot[-1]
    else:
        assert y[0] == -absdot[0] and y[-1] == absdot[-1]
    assert np.all(np.diff(y) > 0)
    assert np.abs(y).min() < 0.05 * absdot.max()
    assert 32752 <= absdot.max() < 65504          # c is the LARGEST power of two that fits


@pytest.mark.parametrize("cbid,scale", H.CODEBOOKS, ids=IDS)
def test_only_the_overflow_kind_leaves_fp16(cbid, scale):
    L = H.make_aligned_layer(cbid, 4096, 64, scale)
    for kind, col in [(kd, 511) for kd in H.KINDS] + [("onehot", c) for c in H.ONEHOT_COLS]:
        y, _, _ = H.model_of(L, H.activation(L, kind, col=col)[0])
        if kind == "overflow":
            assert np.isposinf(y[-1]) and np.isneginf(y[0]) and np.isfinite(y[L.n // 2])
            assert 0 < np.isinf(y).sum() < L.n
        else:
            assert np.all(np.isfinite(y)), kind
        assert not np.any(np.isnan(y))


def test_planes_of_fp16_digits():
    """X = 2^22 - 2^11 is (64, -8, 0); the digits are balanced and recompose; a subnormal counts as exponent -14"""
    h, m, l, sh = H.planes_of_fp16(np.array([(2 - 2.0 ** -10) * 4, -1.0], np.float16))
    assert sh == 21 - 2 and (h[0], m[0], l[0]) == (64, -8, 0) and (h[1], m[1], l[1]) == (-8, 0, 0)
    X = np.arange(-2 ** 22 + 1, 2 ** 22, 4099)
    h, m, l = H.digits_of(X)
    assert np.array_equal(h * 65536 + m * 256 + l, X)
    assert np.all((-128 <= m) & (m < 128) & (-128 <= l) & (l < 128) & (-64 <= h) & (h <= 64))
    h, m, l, sh = H.planes_of_fp16(np.full(8, 2.0 ** -24, np.float16))
    assert sh == 35 and np.all(h * 65536 + m * 256 + l == 2 ** 11)
    assert H.planes_of_fp16(np.zeros(8, np.float16))[3] == 35


@pytest.mark.parametrize("k", [512, 4096, 28672])
@pytest.mark.parametrize("cbid,scale", H.CODEBOOKS, ids=IDS)
def test_model_against_float64(cbid, scale, k):
    """the model is within _mm_tol of the float64 product of the same (virtual) operands on every kind; where the block
    fixed point holds every element of x exactly (flat, flat_top, tiers, overflow) it IS fp16(y64), infinities included.
    The virtual vectors of the RVQ codebooks with |s| != 1 carry fp16(s x): on `tiers` their small elements are below the
    fixed-point step, so there only _mm_tol holds; `outlier` and `top_mix` may differ from fp16(y64) in a few rows
    (fixed point, double rounding, fl32 of a sum beyond 2^24) and are held to _mm_tol."""
    n = 64
    L = H.make_aligned_layer(cbid, k, n, scale)
    worst = 0.0
    for kind in H.KINDS:
        x, c = H.activation(L, kind, col=k - 1)
        y, smax, xv = H.model_of(L, x)
        assert smax < 2 ** 31, (kind, smax)
        x64 = xv.astype(np.float64)[None, :]
        y64 = x64 @ L.W64.T
        with np.errstate(over="ignore"):
            y16 = y64[0].astype(np.float16)
        # (s = -1: fp16(s x) = -x, the virtual vector is as exact as x)
        exact = kind in H.EXACT_KINDS and not (kind == "tiers" and "RVQ" in cbid and abs(H.fp16_scale(scale)) != 1.0)
        if exact or kind == "onehot":
            assert np.array_equal(y.view(np.uint16), y16.view(np.uint16)), (kind, int((y != y16).sum()))
        if kind != "overflow":
            ratio = np.abs(y.astype(np.float64) - y64[0]) / _mm_tol(x64, L.W64, y64)[0]
            assert ratio.max() <= 1.0, (kind, ratio.max())
            worst = max(worst, float(ratio.max()))
    print(f"{cbid} {scale} k={k}: worst error / tolerance {worst:.3f}")


def test_integer_sums_stay_in_int32_at_every_gpu_shape():
    """max |S_d| < 2^31 at every shape and codebook of tests/test_gpu_product_hard_cases.py, with the factor 8 of the
    nibble mode (E8P12's K-splitting kernel) and the 2k-wide virtual rows included.  Without that factor the sums are
    below 2^24 -- fp32 values -- everywhere but on the 57344-wide virtual rows (HI 2^24.7), where product_model's
    fl32(S_d) is a rounding of its own"""
    top = top24 = (0, None)
    for cbid, scale in H.CODEBOOKS:
        for k in H.SHAPES[cbid]:
            for n in (37,) if k > 4096 else (37, 257):
                L = H.make_aligned_layer(cbid, k, n, scale)
                for kind in ("flat", "flat_top", "tiers", "top_mix", "outlier", "overflow"):
                    smax = H.model_of(L, H.activation(L, kind)[0])[1]
                    # the sums are fp32 values (below 2^24) wherever the row is not one of the 57344-wide virtual rows
                    assert smax < 2 ** 24 or L.kv == 57344, (cbid, k, kind, smax)
                    top24 = max(top24, (smax, (cbid, scale, n, k, kind)))
                    smax *= 8 if cbid == "E8P12" else 1
                    assert smax < 2 ** 31, (cbid, k, kind, smax)
                    top = max(top, (smax, (cbid, scale, n, k, kind)))
    n, k = H.V2_DYNAMIC
    L = H.make_aligned_layer("E8P12", k, n)
    smax = 8 * H.model_of(L, H.activation(L, "flat_top")[0])[1]
    assert smax < 2 ** 31
    top = max(top, (smax, ("E8P12", None, n, k, "flat_top")))
    assert top24[0] > 2 ** 24          # the range beyond fp32's integers IS reached
    print(f"largest |S_d| without the factor: {top24[0]} = 2^{np.log2(top24[0]):.2f} at {top24[1]}")
    print(f"largest |S_d| (x 8 in nibble mode): {top[0]} = 2^{np.log2(top[0]):.2f} at {top[1]}")
