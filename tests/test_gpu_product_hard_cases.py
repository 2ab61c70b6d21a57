"""The quantised products on the inputs of tests/product_hard_cases.py (run with -m gpu on an MI355X): codes aligned to
the sign of x, activations that are flat, at the top of the fixed-point range, tiered by digit plane, dominated by one
outlier, one-hot, subnormal, or large enough to overflow fp16 -- instead of randn against random codes, whose integer
sums stay thirty times below what a sign-aligned row reaches.

The integer-domain paths are held to the BITS of product_model(), fed with the digit planes read back from
the device so that the check is of the product alone; the planes themselves are checked against planes_of_fp16().  The
one exception is the VALU kernel (csrc/e8p_gemv_i8.hip, kernels 0 and 3 of quip_e8p_gemv_tuned): its epilogue is
documented as ordered differently -- every lane combines its three digit sums in fp32 and the lanes and K slices are
then added in fp32 -- so it is held to adjacent fp16 values (one ulp) of the model.  The fp16-domain paths (generic mm,
single-pass skinny kernel, prefill GEMM) are held to tests.test_gpu_ops._mm_tol against float64."""
import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from tests import product_hard_cases as H
from tests.test_gpu_gemv_v2 import VARIANTS
from tests.test_gpu_ops import DEV, _cb, _mm_tol

pytestmark = pytest.mark.gpu

IDS = [f"{c}{'' if s is None else f'_{s:+.2f}'}" for c, s in H.CODEBOOKS]
NAN16 = float("nan")


@pytest.fixture(scope="module")
def Q():
    assert torch.cuda.is_available()
    import quip_for_all_amd as Q
    return Q


def _lib():
    from quip_for_all_amd import capi
    return capi.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _linear_planes(xv, out=None):
    """quip_e8p_x_to_planes of an fp16 vector -> the uint8 image (three planes of Kp digits, the shift word)"""
    L = _lib()
    k = xv.shape[-1]
    xd = _dev(xv.reshape(1, k))
    planes = torch.empty(L.quip_e8p_planes_bytes(k), dtype=torch.uint8, device=DEV) if out is None else out
    assert L.quip_e8p_x_to_planes(xd.data_ptr(), planes.data_ptr(), k, _stream()) == 0
    return planes


def _read_linear(planes, k):
    """the image as _decode_planes of tests/test_gpu_ops.py reads it, digit by digit -> (h, m, l, sh, padding)"""
    kp = (k + 511) // 512 * 512
    p = planes.cpu().numpy()
    d = p[:3 * kp].reshape(3, kp).view(np.int8).astype(np.int64)
    sh = int(p[3 * kp:3 * kp + 4].view(np.int32)[0])
    return d[0, :k], d[1, :k], d[2, :k], sh, d[:, k:]


def _read_laneorder(planes, k):
    """quip_e8p_x_to_planes_laneorder: 8-byte units [(c * 3 + d) * slices + lp] hold digit d of the elements
    [8 (8 lp + c), + 8); the shift word follows the 3 k digits"""
    p = planes.cpu().numpy()
    d = p[:3 * k].view(np.int8).reshape(8, 3, k // 64, 8).transpose(1, 2, 0, 3).reshape(3, k).astype(np.int64)
    return d[0], d[1], d[2], int(p[3 * k:3 * k + 4].view(np.int32)[0])


def _ordinal(y):
    """fp16 values on the integer line on which adjacent values differ by one (+-0 = 0, inf follows 65504)"""
    b = np.asarray(y, dtype=np.float16).view(np.uint16).astype(np.int64)
    return np.where(b & 0x8000, -(b & 0x7FFF), b & 0x7FFF)


def _cases(L, cols=(511,)):
    """(name, x) of every kind, the one-hot kind at each of `cols`"""
    out = []
    for kind in H.KINDS:
        if kind == "onehot":
            out += [(f"onehot@{c % L.k}", H.activation(L, kind, col=c)[0]) for c in cols]
        else:
            out.append((kind, H.activation(L, kind)[0]))
    return out


def _expect(L, planes):
    """the model on the planes the device wrote -> (y, max |S_d|)"""
    h, m, l, sh, pad = _read_linear(planes, L.kv)
    assert not pad.any()
    y, smax = H.product_model(h, m, l, sh, L.W_int, L.log2_unit)
    return y, smax


def _onehot_column(L, x):
    with np.errstate(over="ignore"):
        return (L.W64 @ H.virtual_x(L.cbid, x, L.scale).astype(np.float64)).astype(np.float16)


def _same_bits(got, want, what):
    g = got.detach().cpu().numpy().reshape(-1).view(np.uint16)
    w = np.asarray(want, dtype=np.float16).reshape(-1).view(np.uint16)
    assert g.shape == w.shape and np.array_equal(g, w), (what, int((g != w).sum()), np.flatnonzero(g != w)[:8])


# ------------------------------------------------------------------------------------------------------------------
# digit planes from fp16
# ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", H.SHAPES["E8P12"])
def test_digit_planes_from_fp16(k):
    """quip_e8p_x_to_planes and quip_e8p_x_to_planes_laneorder == planes_of_fp16 in every digit and in sh, on every kind
    and on the virtual vectors of HI (zeros between the elements) and RVQ4B (the residual half scaled); the padding
    [k, Kp) of the linear image is zero"""
    L = _lib()
    vectors = list(_cases(H.make_aligned_layer("E8P12", k, 37), H.ONEHOT_COLS))
    for cbid, scale in (("HI", None), ("E8P12RVQ4B", -1.0), ("E8P12RVQ4B", 1 / 3.45)):
        Lv = H.make_aligned_layer(cbid, k, 37, scale)
        vectors += [(f"{cbid}:{kind}", H.virtual_x(cbid, H.activation(Lv, kind)[0], scale))
                    for kind in ("flat_top", "tiers", "outlier")]
    top = 0
    for name, xv in vectors:
        kv = xv.shape[0]
        h, m, l, sh = H.planes_of_fp16(xv)
        gh, gm, gl, gsh, pad = _read_linear(_linear_planes(xv), kv)
        assert gsh == sh and not pad.any(), (name, gsh, sh)
        assert np.array_equal(gh, h) and np.array_equal(gm, m) and np.array_equal(gl, l), name
        lo = torch.full((3 * kv + 16,), 0x55, dtype=torch.uint8, device=DEV)
        assert L.quip_e8p_x_to_planes_laneorder(_dev(xv.reshape(1, kv)).data_ptr(), lo.data_ptr(), kv, _stream()) == 0
        gh, gm, gl, gsh = _read_laneorder(lo, kv)
        assert gsh == sh, (name, "lane order", gsh, sh)
        assert np.array_equal(gh, h) and np.array_equal(gm, m) and np.array_equal(gl, l), (name, "lane order")
        top = max(top, int(np.abs(h * 65536 + m * 256 + l).max()))
    print(f"k={k}: {len(vectors)} vectors, every digit and sh equal; largest |X| = {top} (2^22 = {2 ** 22})")


# ------------------------------------------------------------------------------------------------------------------
# integer-domain products: bits of the model
# ------------------------------------------------------------------------------------------------------------------

# quip_e8p_gemv_tuned: (kernel, rep, rows, blocks, g, maxw, digits) -- 4: matrix-core GEMV on linear planes,
# 0: VALU integer GEMV on lane-ordered planes, 3: the same converting x itself
FIRST_KERNELS = [(4, 0, 0, 0, 0, 0, 0), (4, 16, 2, 0, 0, 16, 0), (4, 0, 3, 3, 0, 12, 0),
                 (0, 1, 2, 0, 0, 16, 3), (0, 32, 2, 0, 0, 16, 3), (0, 32, 4, 64, 2, 0, 3),
                 (3, 32, 2, 0, 0, 16, 3), (3, 1, 2, 0, 0, 8, 3)]


@pytest.mark.parametrize("n", H.NS)
@pytest.mark.parametrize("k", H.SHAPES["E8P12"])
def test_e8p_gemv_kernels_4_0_3(Q, n, k):
    """quip_e8p_gemv_tuned: the matrix-core kernel (4) gives the model's bits; the VALU kernel (0 on lane-ordered planes,
    3 converting x itself) adds per-lane fp32 combinations in fp32 -- another order than the model's two fused
    multiply-adds on the exact sums -- and is held to adjacent fp16 values of the model"""
    L = _lib()
    Ly = H.make_aligned_layer("E8P12", k, n)
    Qd = _dev(Ly.Qidxs)
    grid = _cb(Q, "E8P12").grid_packed_abs
    worst_ulp, smax_top, launches = 0, 0, 0
    for name, x in _cases(Ly, H.ONEHOT_COLS):
        xd = _dev(x.reshape(1, k))
        planes = _linear_planes(x)
        want, smax = _expect(Ly, planes)
        smax_top = max(smax_top, smax)
        if name.startswith("onehot"):
            _same_bits(torch.from_numpy(want), _onehot_column(Ly, x), name)
        lo = torch.empty(3 * k + 16, dtype=torch.uint8, device=DEV)
        assert L.quip_e8p_x_to_planes_laneorder(xd.data_ptr(), lo.data_ptr(), k, _stream()) == 0
        for var in FIRST_KERNELS:
            kernel = var[0]
            xin = {4: planes, 0: lo, 3: xd}[kernel]
            y = torch.full((1, n), NAN16, dtype=torch.float16, device=DEV)
            assert L.quip_e8p_gemv_tuned(xin.data_ptr(), Qd.data_ptr(), grid.data_ptr(), y.data_ptr(), n, k, *var, None,
                                         _stream()) == 0, var
            launches += 1
            if kernel == 4 or name.startswith("onehot"):
                _same_bits(y, want, (name, var))          # (a one-hot row has one term: no order to differ in)
            else:
                g = y.cpu().numpy().reshape(-1)
                assert not np.isnan(g).any(), (name, var)
                d = np.abs(_ordinal(g) - _ordinal(want))
                worst_ulp = max(worst_ulp, int(d.max()))
                assert d.max() <= 1, (name, var, int(d.max()), int(d.argmax()))
    print(f"E8P12 {n}x{k}: {launches} launches; kernel 4 bit identical to the model, VALU kernel within {worst_ulp} "
          f"fp16 ulp; max |S_d| = {smax_top}")


def _v2_check(Q, n, k, kinds_cols, variants):
    L = _lib()
    Ly = H.make_aligned_layer("E8P12", k, n)
    Qd = _dev(Ly.Qidxs)
    grid = _cb(Q, "E8P12").grid_packed_abs
    ws = torch.zeros(L.quip_e8p_gemv_v2_workspace_bytes(n) // 4, dtype=torch.int32, device=DEV)
    smax_top, launches = 0, 0
    for name, x in kinds_cols:
        planes = _linear_planes(x)
        want, smax = _expect(Ly, planes)
        smax_top = max(smax_top, smax)
        if name.startswith("onehot"):
            _same_bits(torch.from_numpy(want), _onehot_column(Ly, x), name)
        for var in variants:
            rep, slots, blocks, ksplit, maxw, runlen = var
            if ksplit > (k + 1023) // 1024:
                continue                                   # more K parts than 1024-k segments: the entry refuses
            y = torch.full((1, n), NAN16, dtype=torch.float16, device=DEV)
            assert L.quip_e8p_gemv_v2_tuned(planes.data_ptr(), Qd.data_ptr(), grid.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                            n, k, rep, slots, blocks, ksplit, maxw, runlen, None, _stream()) == 0, var
            launches += 1
            _same_bits(y, want, (name, var))
    assert int(ws.abs().max()) == 0, "workspace must be left zeroed"
    print(f"E8P12 v2 {n}x{k}: {launches} launches bit identical to the model, workspace zero; max |S_d| = {smax_top} "
          f"(x 8 in nibble mode: 2^{np.log2(8 * smax_top):.2f})")


@pytest.mark.parametrize("n", H.NS)
@pytest.mark.parametrize("k", H.SHAPES["E8P12"])
def test_e8p_gemv_v2_variants(Q, n, k):
    """quip_e8p_gemv_v2_tuned over the variant list of tests/test_gpu_gemv_v2.py: byte and nibble tables, forced K
    splits of 2 and 3 (atomics into the workspace, left zeroed), run lengths 1..3"""
    _v2_check(Q, n, k, _cases(H.make_aligned_layer("E8P12", k, n), H.ONEHOT_COLS), VARIANTS)


def test_e8p_gemv_v2_dynamic_runs(Q):
    """(2048, 14336): the waves pull (row quad, K run) items from the counter and flush by difference"""
    n, k = H.V2_DYNAMIC
    Ly = H.make_aligned_layer("E8P12", k, n)
    cases = [c for c in _cases(Ly, (k - 1,)) if c[0] in ("flat_top", "tiers", "outlier", "overflow", f"onehot@{k - 1}")]
    _v2_check(Q, n, k, cases, VARIANTS)


def _mm_planes_shapes():
    return [pytest.param(c, s, k, id=f"{i}-{k}") for (c, s), i in zip(H.CODEBOOKS, IDS) for k in H.SHAPES[c]]


@pytest.mark.parametrize("n", H.NS)
@pytest.mark.parametrize("cbid,scale,k", _mm_planes_shapes())
def test_mm_planes_and_group_every_codebook(Q, cbid, scale, k, n):
    """mm_planes / mm_planes_group of every codebook (the op's dispatcher over the first kernel, the K-splitting kernel
    and its table modes; E8P12RVQ3B always through its workspace entry) on the planes of the virtual vector"""
    cb = _cb(Q, cbid, scale)
    Ly = H.make_aligned_layer(cbid, k, n, scale)
    Qd = _dev(Ly.Qidxs)
    two = cb.planes_group_supported([n, n], k)
    smax_top, prev = 0, None
    for name, x in _cases(Ly, H.ONEHOT_COLS):
        planes = _linear_planes(H.virtual_x(cbid, x, scale))
        want, smax = _expect(Ly, planes)
        smax_top = max(smax_top, smax)
        if name.startswith("onehot"):
            _same_bits(torch.from_numpy(want), _onehot_column(Ly, x), name)
        _same_bits(cb.mm_planes(planes, Qd), want, (name, "mm_planes"))
        if two and prev is not None:                      # two problems with different x in one launch
            ys = cb.mm_planes_group([prev[0], planes], [Qd, Qd])
            _same_bits(ys[0], prev[1], (name, "group[0]"))
            _same_bits(ys[1], want, (name, "group[1]"))
        else:
            _same_bits(cb.mm_planes_group([planes], [Qd])[0], want, (name, "group of one"))
        prev = (planes, want)
    ws = Q.register_lib._GEMV_WS[("cuda", 0, _stream())]
    assert int(ws.abs().max()) == 0
    print(f"{cbid} {scale} {n}x{k} (virtual {Ly.kv}): mm_planes and group{' of two' if two else ''} bit identical to "
          f"the model on {len(H.KINDS) + len(H.ONEHOT_COLS) - 1} inputs; max |S_d| = {smax_top}")


@pytest.mark.parametrize("M", [2, 5, 6])
@pytest.mark.parametrize("n,k", [(37, 512), (257, 1152), (257, 4096), (37, 11008), (37, 28672)])
@pytest.mark.parametrize("cbid,scale", H.CODEBOOKS, ids=IDS)
def test_rows_mode_with_a_different_kind_in_every_row(Q, cbid, scale, n, k, M):
    """rows mode (up to five activation rows per pass over the codes, (row, digit plane) -> A row 3 r + d; virtual rows
    of 57344: one K-splitting launch per row): every row of one call holds another kind, each must come out as the
    model's bits for ITS planes.  M = 6 is followed by a call whose six rows are one-hot at the six columns."""
    L = _lib()
    cb = _cb(Q, cbid, scale)
    Ly = H.make_aligned_layer(cbid, k, n, scale)
    Qd = _dev(Ly.Qidxs)
    every = _cases(Ly, H.ONEHOT_COLS)
    kinds = [c for c in every if not c[0].startswith("onehot")]
    calls = [[kinds[(M + r) % len(kinds)] for r in range(M)]]
    if M == 6:
        calls.append([c for c in every if c[0].startswith("onehot")])
    for cases in calls:
        rows = len(cases)
        planes = torch.empty((rows, L.quip_e8p_planes_bytes(Ly.kv)), dtype=torch.uint8, device=DEV)
        want = []
        for r, (name, x) in enumerate(cases):
            _linear_planes(H.virtual_x(cbid, x, scale), out=planes[r])
            want.append(_expect(Ly, planes[r])[0])
            if name.startswith("onehot"):
                _same_bits(torch.from_numpy(want[r]), _onehot_column(Ly, x), name)
        y = cb.mm_planes_rows(planes, Qd)
        assert y.shape == (rows, n)
        for r, (name, _) in enumerate(cases):
            _same_bits(y[r], want[r], (name, r))
        print(f"{cbid} {scale} {n}x{k} M={rows}: rows {[c[0] for c in cases]} bit identical to the model")


# ------------------------------------------------------------------------------------------------------------------
# fp16-domain products: _mm_tol against float64
# ------------------------------------------------------------------------------------------------------------------

def _batch(Ly, M):
    cases = _cases(Ly, (0, 7, 8, 511, 512, Ly.k - 1))
    return [cases[r % len(cases)] for r in range(M)]


def _check_fp16_domain(y, x, W64, what, xbits):
    """|y - y64| <= _mm_tol (the fixed-point term dropped where the path has none: xbits = None); a float64 result
    that rounds to +-inf in fp16 must be +-inf of that sign, nothing is NaN, and nothing finite in float64 beyond the
    tolerance of 65520 comes out infinite"""
    g = y.detach().cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    y64 = x64 @ W64.T
    tol = _mm_tol(x64, W64, y64, xbits=22 if xbits else 200)
    assert not np.isnan(g).any(), what
    must_inf = np.abs(y64) - tol >= 65520.0
    assert np.all(np.isinf(g[must_inf]) & (np.sign(g[must_inf]) == np.sign(y64[must_inf]))), what
    may_inf = np.abs(y64) + tol >= 65520.0
    assert not np.any(np.isinf(g) & ~may_inf), what
    fin = np.isfinite(g)
    ratio = (np.abs(g - y64) / tol)[fin]
    assert ratio.max() <= 1.0, (what, float(ratio.max()), np.argwhere((np.abs(g - y64) > tol) & fin)[:4])
    return float(ratio.max())


def _fp16_shapes(ks_of):
    return [pytest.param(c, s, k, id=f"{i}-{k}") for (c, s), i in zip(H.CODEBOOKS, IDS) for k in ks_of(c)]


@pytest.mark.parametrize("M", [1, 4])
@pytest.mark.parametrize("n", H.NS)
@pytest.mark.parametrize("cbid,scale,k", _fp16_shapes(lambda c: (512, 1152, 4096, 11008, 28672)))
def test_generic_mm(Q, cbid, scale, k, n, M):
    """cb.mm (the reference's *_mm_origorder ops): fp32 VALU kernels of csrc/codebook_kernels.hip for D4 / HI / RVQ --
    no fixed point --, the block-fixed-point GEMV and rows mode for E8P12"""
    Ly = H.make_aligned_layer(cbid, k, n, scale)
    cb = _cb(Q, cbid, scale)
    W64 = O.decompress(cbid, Ly.Qidxs, 0.0 if scale is None else scale).astype(np.float64)
    Qd = _dev(Ly.Qidxs)
    worst = 0.0
    cases = _cases(Ly, H.ONEHOT_COLS)
    for i in range(0, len(cases), M):
        x = np.stack([c[1] for c in cases[i:i + M]])
        y = cb.mm(_dev(x), Qd)
        worst = max(worst, _check_fp16_domain(y, x, W64, (cbid, [c[0] for c in cases[i:i + M]]), cbid == "E8P12"))
        for r, (name, xr) in enumerate(cases[i:i + M]):
            if name.startswith("onehot"):
                col = int(np.flatnonzero(xr)[0])
                with np.errstate(over="ignore"):
                    _same_bits(y[r], (W64[:, col] * float(xr[col])).astype(np.float16), name)
    print(f"{cbid} {scale} mm {n}x{k} M={M}: worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("M", [6, 31, 33])
@pytest.mark.parametrize("n", [38, 258])
@pytest.mark.parametrize("cbid,scale,k", _fp16_shapes(lambda c: (512, 1152, 4096, 11008, 28672)))
def test_skinny_kernel(Q, cbid, scale, k, n, M):
    """the single-pass fp16 skinny kernel (exact fp16 weights, fp32 accumulation, no fixed point); it takes even n
    only, so n = 38 / 258 stand for 37 / 257 here; M = 33 is two chunks"""
    Ly = H.make_aligned_layer(cbid, k, n, scale)
    cb = _cb(Q, cbid, scale)
    W64 = O.decompress(cbid, Ly.Qidxs, 0.0 if scale is None else scale).astype(np.float64)
    cases = _batch(Ly, M)
    x = np.stack([c[1] for c in cases])
    y = cb.mm_skinny(_dev(x), _dev(Ly.Qidxs))
    worst = _check_fp16_domain(y, x, W64, (cbid, k, M), False)
    for r, (name, xr) in enumerate(cases):
        if name.startswith("onehot"):
            col = int(np.flatnonzero(xr)[0])
            _same_bits(y[r], (W64[:, col] * float(xr[col])).astype(np.float16), name)
    print(f"{cbid} {scale} skinny {n}x{k} M={M}: worst error / tolerance {worst:.3f}")


@pytest.mark.parametrize("M", [32, 40])
@pytest.mark.parametrize("n", [38, 258])
@pytest.mark.parametrize("cbid,scale,k", _fp16_shapes(lambda c: (512, 1152, 4096, 11008, 28672)))
def test_prefill_gemm(Q, cbid, scale, k, n, M):
    """the fused dequant + MFMA tile kernel (mm_batched; even n, k % 64 == 0: n = 38 / 258 stand for 37 / 257)"""
    Ly = H.make_aligned_layer(cbid, k, n, scale)
    cb = _cb(Q, cbid, scale)
    W64 = O.decompress(cbid, Ly.Qidxs, 0.0 if scale is None else scale).astype(np.float64)
    cases = _batch(Ly, M)
    x = np.stack([c[1] for c in cases])
    Qd = _dev(Ly.Qidxs)
    if cbid == "E8P12":
        y = torch.ops.quip_lib.e8p_mm_batched(_dev(x), Qd, cb.grid_packed_abs)
    else:
        y = cb.mm_batched(_dev(x), Qd)
    worst = _check_fp16_domain(y, x, W64, (cbid, k, n, M), False)
    for r, (name, xr) in enumerate(cases):
        if name.startswith("onehot"):
            col = int(np.flatnonzero(xr)[0])
            _same_bits(y[r], (W64[:, col] * float(xr[col])).astype(np.float16), name)
    print(f"{cbid} {scale} prefill {n}x{k} M={M}: worst error / tolerance {worst:.3f}")
