"""The input transforms that write digit planes (had_transform_planes, its _rows form, the chain and fused launches) at
BOTH ends of the norm bound (run with -m gpu on an MI355X).  For K > 1 the planes' block exponent comes from
|x|_2 sqrt(L) |scale| 1.0625, not from the maximum: randn sits 4-5 bits under it.

    flat_row   x = row_j(M) / su, M the full transform: the output is ONE spike, as large as the bound allows
    onehot     the output is flat: as far under the bound as an output can be (sqrt(n) under it)
    outlier    |randn| with one element 3000
    randn      for comparison

Every element is held to half a fixed-point step plus the forward error of the fp32 arithmetic, DERIVED, not measured:
    2^(-sh-1) + 2^-23 (K + log2 L + 1) (|M| |x|)_i |scale|
(a K-term mix, log2 L butterfly levels and the scaling, each at fp32 unit roundoff 2^-24, doubled), the virtual
vectors of the RVQ and HI layouts to the same bound applied to x'."""
import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from tests.test_gpu_chain_k import _layer, _separate, _t
from tests.test_gpu_ops import DEV

pytestmark = pytest.mark.gpu

KINDS = ("flat_row", "onehot", "outlier", "randn")
# (n, K of the random orthogonal factor); with the +-1 / sqrt(K) tables of get_hadK(use_rand=False) the same widths are
# 1408 = 44 x 32, 2752 = 172 x 16 (L < 64: had_small_kernel, and so is 352 = 11 x 32 with the random factor),
# 5120 = 20 x 256, 3584 = 28 x 128 (the tall kernel)
WIDTHS = [(1024, 1), (1408, 11), (2752, 43), (5120, 5), (3584, 7), (352, 11)]
HI = float("inf")        # register_lib.HI_PLANES
LAYOUTS = [("plain", 0.0), ("rvq", float(np.float16(1 / 3.45))), ("rvq", -1.0), ("hi", HI)]


@pytest.fixture(scope="module", autouse=True)
def _ops():
    assert torch.cuda.is_available()
    import quip_for_all_amd  # noqa: F401  (registers torch.ops.quip_lib)


def _factor(n, K, table):
    """(had fp16 (K, K) or None, K) -- table 'rand': a random orthogonal factor; 'pm1': get_hadK(n, use_rand=False)"""
    if K == 1:
        return None, 1
    if table == "rand":
        return O.random_orthogonal(K, np.random.default_rng(n + K)).astype(np.float16), K
    from quip_for_all_amd.quant import get_hadK
    had, K2, qn = get_hadK(n, False)
    assert qn == n and K2 > 1
    return had.numpy().astype(np.float16), K2


def _layout_served(K, L, layout):
    """fill() of csrc/hadamard.hip: the virtual layouts are written by the blocked kernels only"""
    return layout == "plain" or L >= 256 or (K > 1 and L >= 64)


def _apply(v, had, K, n, scale, transpose=True):
    return O.matmul_hadU(v, None if had is None else had.astype(np.float64), K, n, scale=scale, transpose=transpose)


def _input(kind, n, K, had, su, seed, j=None):
    """(1, n) fp16.  flat_row: su * x = row_j(M) up to fp16 rounding -- row_j(M) = M^T e_j, and M^T is the same
    transform with the K factor transposed the other way (H_L is symmetric)"""
    rng = np.random.default_rng(seed)
    if kind == "flat_row":
        j = (5 * n) // 7 if j is None else j
        e = np.zeros(n)
        e[j] = 1.0
        r = _apply(e, had, K, n, 1.0, transpose=False)
        x = r / np.abs(r).max() / su.astype(np.float64)
    elif kind == "onehot":
        x = np.zeros(n)
        x[(3 * n) // 11 if j is None else j] = 2.0
    else:
        x = rng.standard_normal(n)
        if kind == "outlier":
            x = np.abs(x)
            x[(7 * n) // 16 + 3] = 3000.0
    return x.astype(np.float16).reshape(1, n)


def _virtual(ref, layout, s):
    """the float64 virtual vector the layout's planes stand for, and the factor on the error bound per element"""
    if layout == "plain":
        return ref
    g = ref.reshape(-1, 8)
    if layout == "rvq":
        return np.concatenate([s * g, g], axis=1).reshape(-1)
    z = np.zeros((g.shape[0], 2))
    return np.concatenate([g[:, [0, 2]], z, g[:, [4, 6]], z, g[:, [1, 3]], z, g[:, [5, 7]], z], axis=1).reshape(-1)


def _decode(planes, nv):
    kp = (nv + 511) // 512 * 512
    p = planes.cpu().numpy()
    d = p[:3 * kp].reshape(3, kp).view(np.int8).astype(np.int64)
    return d[0] * 65536 + d[1] * 256 + d[2], int(p[3 * kp:3 * kp + 4].view(np.int32)[0])


def _check_planes(planes, x, su, had, n, K, scale, layout, s, kind):
    """the assertions of the module docstring on one plane image -> (error / bound, max |X| / 2^21)"""
    L = n // K
    nv = n if layout == "plain" else 2 * n
    X, sh = _decode(planes, nv)
    assert np.all(np.abs(X) < 2 ** 22), (kind, int(np.abs(X).max()))
    assert not X[nv:].any()                                          # k padding
    xs = x[0].astype(np.float64) * su.astype(np.float64)
    ref = _apply(xs, had, K, n, scale * np.sqrt(L))                  # `scale` carries 1 / sqrt(L), as the op takes it
    # (|M| |x|)_i |scale|: |M| = |A| (x) ones(L, L) -- constant over the L elements of a sub-row
    A = np.ones((1, 1)) if had is None else np.abs(had.astype(np.float64).T)
    spread = np.repeat(A @ np.abs(xs).reshape(K, L).sum(1), L) * abs(scale)
    fwd = 2.0 ** -23 * (K + np.log2(L) + 1) * spread
    tol = 2.0 ** (-sh - 1) + _virtual(fwd, layout, abs(s) if layout == "rvq" else 1.0)
    want = _virtual(ref, layout, s)
    got = X[:nv].astype(np.float64) * 2.0 ** -sh
    ratio = np.abs(got - want) / tol
    assert ratio.max() <= 1.0, (kind, layout, float(ratio.max()), int(ratio.argmax()))
    if layout == "hi":
        assert not X[:nv].reshape(-1, 4)[:, 2:].any()               # the zeros between the pairs are zeros
    top = np.abs(X).max() / 2.0 ** 21
    if K == 1:
        assert top >= 1.0, (kind, top)                               # exact maximum
    elif kind == "flat_row":
        assert top >= 1 / 1.07, (kind, top)                          # never a bit looser than the bound requires
    return float(ratio.max()), float(top)


@pytest.mark.parametrize("layout,s", LAYOUTS, ids=["plain", "rvq+0.29", "rvq-1.00", "hi"])
@pytest.mark.parametrize("n,K,table", [(n, K, t) for n, K in WIDTHS for t in ("rand", "pm1") if K > 1 or t == "rand"])
def test_had_transform_planes_at_both_ends_of_the_norm_bound(n, K, table, layout, s):
    had, K = _factor(n, K, table)
    L = n // K
    if not _layout_served(K, L, layout):
        with pytest.raises((ValueError, RuntimeError)):            # refused, not written in the plain layout
            torch.ops.quip_lib.had_transform_planes_fused(torch.zeros(1, n, dtype=torch.float16, device=DEV), n, K,
                                                          None if had is None else _t(had), True, None, 1.0, None, 1e-5,
                                                          None, s)
        return
    rng = np.random.default_rng(n + K)
    su = rng.choice([-1.0, 1.0], n).astype(np.float16)
    scale = 0.37 / np.sqrt(L)
    hd = None if had is None else _t(had)
    xs = np.concatenate([_input(kind, n, K, had, su, seed=n + i) for i, kind in enumerate(KINDS)])
    op = torch.ops.quip_lib
    rows = op.had_transform_planes_rows(_t(xs), n, K, hd, True, _t(su), float(scale), None, 1e-5, None, s)
    out = []
    for i, kind in enumerate(KINDS):
        x = xs[i:i + 1]
        if layout == "plain":
            planes = op.had_transform_planes(_t(x), n, K, hd, True, _t(su), float(scale))
        else:
            planes = op.had_transform_planes_fused(_t(x), n, K, hd, True, _t(su), float(scale), None, 1e-5, None, s)
        r, top = _check_planes(planes, x, su, had, n, K, scale, layout, s, kind)
        used = planes.numel() - 12                                   # (the 12 bytes behind the shift word are nobody's)
        assert torch.equal(rows[i][:used], planes[:used]), (kind, "the _rows form writes the same image")
        out.append(f"{kind} err/bound {r:.3f} max|X|/2^21 {top:.4f}")
    print(f"n={n} K={K} L={L} {table} {layout} s={s}: " + "; ".join(out))


@pytest.mark.parametrize("n,K", [(1408, 11), (5120, 5), (3584, 7), (352, 11)])
def test_every_spike_position_class_of_flat_row(n, K):
    """flat_row at the first and the last output element, and one in every K sub-row: the spike reaches the bound in
    whichever workgroup / thread group holds it"""
    had, K = _factor(n, K, "rand")
    L = n // K
    su = np.random.default_rng(n).choice([-1.0, 1.0], n).astype(np.float16)
    scale = 0.37 / np.sqrt(L)
    tops = []
    for j in [0, n - 1] + [kp * L + (37 * kp) % L for kp in range(K)]:
        x = _input("flat_row", n, K, had, su, seed=j, j=j)
        planes = torch.ops.quip_lib.had_transform_planes(_t(x), n, K, _t(had), True, _t(su), float(scale))
        r, top = _check_planes(planes, x, su, had, n, K, scale, "plain", 0.0, "flat_row")
        X, _ = _decode(planes, n)
        assert int(np.abs(X).argmax()) == j
        tops.append(top)
    print(f"n={n} K={K}: spike at {K + 2} positions, max|X|/2^21 in [{min(tops):.4f}, {max(tops):.4f}]")


# ------------------------------------------------------------------------------------------------------------------
# chain and fused launches: bit identical to the separate launches on the same inputs
# ------------------------------------------------------------------------------------------------------------------

def _consumer_input(kind, l0, seed):
    """the activation the consumers' input transform sees, (1, k) fp16: flat_row is a row of layers[0]'s transform
    divided by its SU"""
    n, K = l0.q_in_features, l0.K_left
    had = None if K == 1 else l0.had_left.detach().cpu().numpy().astype(np.float16)
    su = l0.SU.detach().cpu().numpy().astype(np.float16)
    return _input(kind, n, K, had, su, seed)


def _check_launches(cbid, k, fouts, h_kind, z_kind, with_rms):
    """h = prev's output transform of z + residual: with z = 0 the residual IS the consumers' input (h_kind); with
    z_kind the producer's output side works on a one-hot / outlier z as well"""
    from quip_for_all_amd import qlinear as QL
    layers = [_layer(O.make_layer(cbid, k, fo, seed=k + fo + i)) for i, fo in enumerate(fouts)]
    prev = _layer(O.make_layer(cbid, 512, k, seed=k + 11))
    assert QL.chain_supported(layers, prev)
    rng = np.random.default_rng(k)
    w = _t(1 + 0.1 * rng.standard_normal(k)) if with_rms else None
    res = _t(_consumer_input(h_kind, layers[0], seed=k))
    z = torch.zeros(1, k, dtype=torch.float16, device=DEV) if z_kind is None else \
        _t(_input(z_kind, k, 1, None, np.ones(k, np.float16), seed=k + 1) * 8)
    with torch.no_grad():
        h_ref, planes_ref = _separate(layers, prev, z, res, w)
        if z_kind is None:
            assert torch.equal(h_ref.view(torch.int16), res.view(torch.int16))
        h, planes = QL.chain_planes(layers, prev, z, residual=res, rms_weight=w)
        h2, zs = QL.gemv_chain(layers, prev, z, residual=res, rms_weight=w)
        torch.cuda.synchronize()
        assert torch.equal(h.view(torch.int16), h_ref.view(torch.int16))
        assert torch.equal(h2.view(torch.int16), h_ref.view(torch.int16))
        ys = []
        for l, pl, pr, zf in zip(layers, planes, planes_ref, zs):
            used = pl.numel() - 12
            assert pl.shape == pr.shape and torch.equal(pl[:used], pr[:used])
            y = l.codebook.mm_planes(pr, l.Qidxs)
            assert torch.equal(zf.view(torch.int16), y.view(torch.int16))
            assert torch.isfinite(y.float()).all()
            ys.append(y)
        if cbid == "E8P12" and QL.fused_in_supported(layers, prev=prev):
            h3, zs3 = QL.gemv_fused(layers, prev=prev, z=z, residual=res, rms_weight=w)
            assert torch.equal(h3.view(torch.int16), h_ref.view(torch.int16))
            for zf, y in zip(zs3, ys):
                assert torch.equal(zf.view(torch.int16), y.view(torch.int16))
            _, zs4 = QL.gemv_fused(layers, x=h_ref, rms_weight=w)
            for zf, y in zip(zs4, ys):
                assert torch.equal(zf.view(torch.int16), y.view(torch.int16))
            return "chain + fused"
    return "chain"


@pytest.mark.parametrize("h_kind,z_kind", [("flat_row", None), ("onehot", None), ("outlier", None), ("randn", "onehot"),
                                           ("flat_row", "outlier")])
@pytest.mark.parametrize("k,fouts", [(4096, (4096,)), (4096, (4096, 512, 512)), (5120, (5120, 1024)), (3584, (3584, 512, 512))])
@pytest.mark.parametrize("with_rms", [False, True])
def test_chain_and_fused_launches_bit_identical(k, fouts, h_kind, z_kind, with_rms):
    """gemv_chain (K = 1 at 4096, the K = 5 / 7 chain at 5120 / 3584) and, where the fused prologue takes the shape,
    gemv_fused: h, every byte of every plane image and the GEMV outputs equal the separate transform launch followed by
    the product -- tests/test_gpu_chain_k.py's statement, here on inputs at both ends of the norm bound"""
    what = _check_launches("E8P12", k, fouts, h_kind, z_kind, with_rms)
    print(f"k={k} {fouts} h={h_kind} z={z_kind} rms={with_rms}: {what} bit identical to the separate launches")


@pytest.mark.parametrize("cbid", ["E8P12RVQ4B", "HI", "D4"])
@pytest.mark.parametrize("h_kind", ["flat_row", "onehot"])
def test_chain_plane_layouts_bit_identical(cbid, h_kind):
    what = _check_launches(cbid, 5120, (5120, 1024), h_kind, None, True)
    print(f"{cbid} 5120 h={h_kind}: {what} bit identical to the separate launches")
