"""The fp32 / fp64 incoherence transform on the GPU (csrc/had_wide.hip): torch.ops.quip_lib.had_wide_rows against
quant.matmul_hadU in float64 on the CPU, exact cases, rows independent of the batch, and the quantiser's fused route.
Bound of an element: gamma_m sum_i |s_out_j| |U_ji| |s_in_i x_i|, m = log2 L + K + 3 (one rounding per butterfly stage, a
length-K dot product, the two scales and 1 / sqrt L), u = 2^-24 | 2^-53; fp32 adds 2^-40 of the sum for the reference, fp64
is held to 2 gamma_m since the reference rounds as often.  |H_L| is constant, so the sum is |Hk| applied to the segments'
absolute sums / sqrt L.  QUIP_HAD_WIDE_ERRORS names a file that receives the largest ratio per case
(profiles/had_wide_errors.txt)."""
import functools
import math
import os

import numpy as np
import pytest
import torch
from torch import nn

from quip_for_all_amd import codebook, quant, quip
from quip_for_all_amd.register_lib import had_wide_tile_rows

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "fp64": torch.float64}
RATIOS = {}


@pytest.fixture(scope="module", autouse=True)
def ratios_file():
    yield
    if os.environ.get("QUIP_HAD_WIDE_ERRORS") and RATIOS:
        with open(os.environ["QUIP_HAD_WIDE_ERRORS"], "w") as f:
            f.writelines(f"{k:48s} {v:.4f}\n" for k, v in sorted(RATIOS.items()))


@functools.lru_cache(maxsize=None)
def problem(K, L, hadK_t, integer=False):
    """33 rows, hadK, scales and the float64 reference with its bound's sum, full width; a row's reference is its own"""
    n = K * L
    g = torch.Generator().manual_seed(K * 100003 + L)
    x = torch.randint(-1024, 1025, (33, n), generator=g).double() if integer else torch.randn(33, n, generator=g).double()
    if integer:
        x[1], x[2] = 0, 0
        x[1, n - 1], x[2, 0] = 1, -3                 # one-hot rows
    x = x.float().double()                           # exact in both dtypes
    hadK = torch.linalg.qr(torch.randn(K, K, generator=g))[0].float().contiguous() if K > 1 else None
    s_in, s_out = (torch.randn(n, generator=g).float().double() for _ in range(2))

    @functools.lru_cache(maxsize=None)
    def both(scaled, in_cols):
        z = x[:, :in_cols] * (s_in[:in_cols] if scaled else 1.0)
        ref = quant.matmul_hadU(z, hadK, K, n, transpose=bool(hadK_t))
        a = torch.nn.functional.pad(z.abs(), (0, n - in_cols)).reshape(33, K, L).sum(-1) / math.sqrt(L)      # (33, K)
        if K > 1:
            a = a @ (hadK.double().abs() if hadK_t else hadK.double().abs().T)
        return ref, a.repeat_interleave(L, dim=1)
    return x, hadK, s_in, s_out, both


def run(x64, dtype, K, L, hadK, hadK_t, s_in, s_out, out_cols, store_t, scale=1.0):
    dev = lambda t: None if t is None else t.to("cuda", dtype if t.dtype == torch.float64 else t.dtype).contiguous()   # noqa: E731
    y = torch.ops.quip_lib.had_wide_rows(dev(x64), K * L, K, dev(hadK), bool(hadK_t), dev(s_in), dev(s_out), scale, out_cols,
                                         bool(store_t))
    return (y.T if store_t else y).double().cpu()


@pytest.mark.parametrize("rows_kind", ["one", "tile+1", "33"])
@pytest.mark.parametrize("store_t", [0, 1])
@pytest.mark.parametrize("hadK_t", [0, 1])
@pytest.mark.parametrize("dt", ["fp32", "fp64"])
@pytest.mark.parametrize("K,L", [(1, 64), (1, 4096), (3, 64), (43, 256), (64, 64), (7, 4096)])
def test_op_against_float64(K, L, dt, hadK_t, store_t, rows_kind):
    dtype, n = DTYPES[dt], K * L
    rows = {"one": 1, "tile+1": had_wide_tile_rows(dtype, n) + 1, "33": 33}[rows_kind]
    x, hadK, s_in, s_out, both = problem(K, L, hadK_t)
    u = 2.0 ** -24 if dt == "fp32" else 2.0 ** -53
    m = math.log2(L) + K + 3
    gamma = m * u / (1 - m * u)
    worst = 0.0
    for in_cols, out_cols, si, so, scale in ((n - 5, n, None, None, 1.0), (n, n - 7, s_in, s_out, 0.75),
                                             (n - 8, n - 4, s_in, None, 1.0)):
        ref, sums = both(si is not None, in_cols)
        post = (1.0 if so is None else so[:out_cols].abs()) * scale
        want = ref[:rows, :out_cols] * (1.0 if so is None else so[:out_cols]) * scale
        bound = sums[:rows, :out_cols] * post * (gamma + 2.0 ** -40 if dt == "fp32" else 2 * gamma)
        got = run(x[:rows, :in_cols], dtype, K, L, hadK, hadK_t, None if si is None else si[:in_cols],
                  None if so is None else so[:out_cols], out_cols, store_t, scale)
        assert got.shape == want.shape
        ratio = ((got - want).abs() / bound.clamp(min=1e-300)).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (in_cols, out_cols, ratio)
    RATIOS[f"K={K} L={L} {dt} hadK_t={hadK_t} store_t={store_t} rows={rows}"] = worst


@pytest.mark.parametrize("store_t", [0, 1])
@pytest.mark.parametrize("dt", ["fp32", "fp64"])
@pytest.mark.parametrize("L", [64, 256, 1024])
def test_integer_and_one_hot_rows_are_exact(L, dt, store_t):
    x, _, _, _, both = problem(1, L, 0, integer=True)
    for in_cols, out_cols in ((L, L), (L - 3, L - 6)):
        got = run(x[:, :in_cols], DTYPES[dt], 1, L, None, 0, None, None, out_cols, store_t)
        assert torch.equal(got, both(False, in_cols)[0][:, :out_cols])


@pytest.mark.parametrize("store_t", [0, 1])
@pytest.mark.parametrize("dt", ["fp32", "fp64"])
@pytest.mark.parametrize("K,L", [(1, 4096), (43, 256), (7, 4096)])
def test_rows_do_not_depend_on_the_batch(K, L, dt, store_t):
    x, hadK, s_in, s_out, _ = problem(K, L, 1)
    R = had_wide_tile_rows(DTYPES[dt], K * L)
    go = lambda a: run(a, DTYPES[dt], K, L, hadK, 1, s_in, s_out, K * L, store_t)       # noqa: E731
    assert torch.equal(go(x[:R + 1]), torch.cat((go(x[:1]), go(x[1:R + 1]))))


@pytest.mark.parametrize("rows,columns,fused", [(192, 256, True), (688, 688, False)])
def test_route(rows, columns, fused, monkeypatch):
    torch.manual_seed(3)
    (lhad, lK, lN), (rhad, rK, rN) = quant.get_hadK(columns), quant.get_hadK(rows)
    H, w = torch.randn(columns, columns, device="cuda"), torch.randn(rows, columns, device="cuda")
    H = H @ H.T / columns
    SU, SV = torch.randn(columns, device="cuda").sign(), torch.randn(rows, device="cuda").sign()
    args = (lhad, lK, lN, rhad, rK, rN)
    monkeypatch.setattr(quant, "_INCOHERENCE_FUSED", True)
    assert quant.incoherence_route(H, lK, lN, rK, rN) == ("fused" if fused else "torch")
    Hi, wi = quant.incoherence_in(H, w, SU, SV, *args)
    back = quant.incoherence_out(wi, SU, SV, *args, columns, rows)
    monkeypatch.setattr(quant, "_INCOHERENCE_FUSED", False)
    if not fused:
        Ht, wt = quant.incoherence_in(H, w, SU, SV, *args)
        assert torch.equal(Hi, Ht) and torch.equal(wi, wt)
        assert torch.equal(back, quant.incoherence_out(wt, SU, SV, *args, columns, rows))
        return
    # the bound composed: a row of U has unit length, so an element's absolute sum is at most its input row's length and an
    # earlier side's error reaches it with at most sqrt(n) of that; 2 sides in, 4 with the way back
    c = lambda t: t.double().cpu()                                                     # noqa: E731
    H64, w64 = quant.incoherence_in(c(H), c(w), c(SU), c(SV), *args)
    back64 = quant.incoherence_out(w64, c(SU), c(SV), *args, columns, rows)
    m = 12                                                                             # log2 64 + 3 + 3 = log2 256 + 1 + 3
    gamma = m * 2.0 ** -24 / (1 - m * 2.0 ** -24)
    for got, want, sides in ((Hi, H64, 2), (wi, w64, 2), (back, back64, 4)):
        assert got.shape == want.shape
        assert (c(got) - want).abs().max() <= sides * gamma * math.sqrt(columns) * want.norm()


def test_quant_end_to_end_agrees_between_the_routes(monkeypatch):
    def go(fused):
        torch.manual_seed(11)
        layer = nn.Linear(256, 192, bias=False).cuda()
        q = quip.QUIP(layer, codebook.codebook_id["E8P12"](inference=False).cuda())
        x = torch.randn(1024, 256, device="cuda") @ torch.randn(256, 256, device="cuda")
        q.add_batch(x)
        W, Hm = layer.weight.data.double().clone(), q.H.clone()
        monkeypatch.setattr(quant, "_INCOHERENCE_FUSED", fused)
        torch.manual_seed(12)
        np.random.seed(12)                               # get_hadK draws the 3 x 3 factor from numpy's generator
        attr = q.quant()
        E = W - layer.weight.data.double()
        return attr, torch.trace(E @ Hm @ E.T).item()
    (a0, p0), (a1, p1) = go(False), go(True)
    assert torch.equal(a0["SU"], a1["SU"]) and torch.equal(a0["SV"], a1["SV"]) and a0["left_hadK"] is a1["left_hadK"] is None
    assert torch.equal(a0["right_hadK"], a1["right_hadK"])
    assert p0 > 0 and abs(p1 - p0) <= 0.02 * p0, (p0, p1)
