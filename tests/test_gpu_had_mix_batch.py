"""had_transform_mix_batch (csrc/had_mix_batch.hip): prefill transforms of K x 512 and K x 1024 rows against
O.matmul_hadU in float64 on the same fp16 operands (run with -m gpu on an MI355X).

Every element is held to a bound that is DERIVED, not measured:
    |y - y64| <= 2^-11 |y64| + 2^-24 + 2^-23 (K + log2 L + 4) (|M| |v|)_i |scale| |post_i|
one fp16 rounding, half the smallest subnormal, and the forward error of a K-term mix, log2 L butterfly levels, the
scaling and the three epilogue operations at fp32 unit roundoff 2^-24, doubled (which also covers the 2^-22 of the
hi / lo split of the mix's operand).  (|M| |v|)_i = (|had| or |had^T|) sum_j |v[k, j]| on the element's sub-row.
The largest error / bound ratio a run shows is printed; profiles/had_mix_batch_errors.txt records it."""
import math

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# K, L, rows: one H tile at the smallest batch; two tiles, one row past a multiple; more rows than any resident grid
# (the row loop and the prefetch wrap); the row buffer at its limit (table factor); three tiles; no padding row in H
SHAPES = [(9, 512, 32), (17, 1024, 33), (27, 512, 600), (28, 1024, 40), (37, 512, 64), (48, 512, 32)]
SIDES = ("plain", "in", "out")


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert torch.cuda.is_available()
    import quip_for_all_amd  # noqa: F401  (registers torch.ops.quip_lib)


def _t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _factor(K, L):
    if (K, L) == (28, 1024):
        from quip_for_all_amd.quant import get_hadK
        had, K2, qn = get_hadK(28672, False)
        assert (K2, qn) == (28, 28672)
        return had.numpy().astype(np.float16)
    return O.random_orthogonal(K, np.random.default_rng(K * L)).astype(np.float16)


def _problem(K, L, rows, side, seed=0):
    """the op's operands as fp16 numpy arrays (None where absent), its sizes and transpose"""
    n = K * L
    rng = np.random.default_rng(seed + n + rows)
    fin = n - 24 if side == "in" else n
    fout = n - 40 if side == "out" else n
    f16 = lambda *s: rng.standard_normal(s).astype(np.float16)  # noqa: E731
    x = f16(rows, fin)
    x[rows // 2] = np.abs(x[rows // 2])
    x[rows // 2, (7 * fin) // 16 + 3] = 3000.0                       # one outlier among |randn|
    p = dict(x=x, had=_factor(K, L), pre=None, gate=None, post=None, bias=None, residual=None)
    if side == "in":
        p.update(pre=f16(fin), gate=f16(rows, fin))
    if side == "out":
        p.update(post=f16(fout), bias=f16(fout), residual=f16(rows, fout))
    return p, n, fin, fout, side == "in", 0.75 / math.sqrt(L)


def _run(p, n, fout, K, transpose, scale, rows=slice(None)):
    row = lambda a: None if a is None else a[rows]  # noqa: E731
    y = torch.ops.quip_lib.had_transform_mix_batch(_t(p["x"][rows]), fout, n, K, _t(p["had"]), transpose, _t(p["pre"]), None,
                                                   _t(p["post"]), _t(p["bias"]), scale, _t(row(p["residual"])), _t(row(p["gate"])))
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("K,L,rows", SHAPES)
def test_against_float64(K, L, rows, side):
    p, n, fin, fout, transpose, scale = _problem(K, L, rows, side)
    y = _run(p, n, fout, K, transpose, scale)
    assert tuple(y.shape) == (rows, fout) and y.dtype == torch.float16
    d = lambda a: a.astype(np.float64)  # noqa: E731
    v = d(p["x"])
    if side == "in":
        g = d(p["gate"])
        v = v * (g / (1.0 + np.exp(-g))) * d(p["pre"])
    had = d(p["had"])
    ref = O.matmul_hadU(v, had, K, n, scale=scale * math.sqrt(L), transpose=transpose)[:, :fout]
    A = np.abs(had.T if transpose else had)
    vp = np.pad(np.abs(v), [(0, 0), (0, n - fin)]).reshape(rows, K, L).sum(2)
    spread = np.repeat(vp @ A.T, L, axis=1)[:, :fout] * abs(scale)
    if side == "out":
        ref = ref * d(p["post"]) + d(p["bias"]) + d(p["residual"])
        spread = spread * np.abs(d(p["post"]))
    bound = 2.0 ** -11 * np.abs(ref) + 2.0 ** -24 + 2.0 ** -23 * (K + math.log2(L) + 4) * spread
    ratio = np.abs(d(y.cpu().numpy()) - ref) / bound
    print(f"had_mix_batch K={K} L={L} rows={rows} {side}: max error / bound {ratio.max():.4f}")
    assert ratio.max() <= 1.0, (np.unravel_index(ratio.argmax(), ratio.shape), ratio.max())


@pytest.mark.parametrize("side", SIDES)
def test_rows_are_independent_bit_for_bit(side):
    K, L, rows = 27, 512, 600
    p, n, fin, fout, transpose, scale = _problem(K, L, rows, side)
    full = _run(p, n, fout, K, transpose, scale)
    assert torch.equal(full, _run(p, n, fout, K, transpose, scale))
    part = _run(p, n, fout, K, transpose, scale, slice(8, 40))
    assert tuple(part.shape) == (32, fout) and torch.equal(part, full[8:40])


def test_quantlinear_prompt_pass_takes_the_new_op(monkeypatch):
    import quip_for_all_amd as Q
    from quip_for_all_amd import register_lib as R
    calls = []
    inner = R._had_transform_mix_batch_cuda
    monkeypatch.setattr(R, "_HAD_MIX_BATCH", True)
    monkeypatch.setattr(R, "_had_transform_mix_batch_cuda", lambda *a, **k: (calls.append(a[2:4]), inner(*a, **k))[1])
    P = O.make_layer("E8P12", 13824, 256, seed=5)
    layer = Q.QuantLinear.from_params(P).to(DEV).eval()
    x = np.random.default_rng(11).standard_normal((64, 13824)).astype(np.float16)
    with torch.no_grad():
        y = layer(_t(x)).cpu().numpy().astype(np.float64)
    assert calls == [(13824, 27)]
    What = O.qlinear_dense_weight(P)
    err = np.abs(y - O.qlinear_forward(P, x, "exact", What))
    assert np.all(err <= O.ulp_bound(P, x, What)), err.max()
