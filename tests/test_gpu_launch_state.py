"""Launch state per kernel (csrc/launch.hip.h) on the GPU: the dynamic-LDS limit of a kernel that several call sites
launch with different sizes, and one launch of every family that moved onto the launch helper, at the smallest shapes
each accepts, against the oracle."""
import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from tests.test_gpu_gemv_v2 import _setup
from tests.test_gpu_ops import DEV, _cb, _decode_planes, _mm_tol

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    assert torch.cuda.is_available()
    import quip_for_all_amd as Q
    return Q


def _transform(planes, x, su, had, n, K):
    """one row through had_fast_kernel<planes, false, 1024>; checked with the bounds of tests/test_gpu_ops.py
    (test_matmul_hadU_cuda for fp16 output, test_had_transform_planes for digit planes)"""
    from quip_for_all_amd import quant
    hd = None if had is None else torch.from_numpy(had).to(DEV)
    if not planes:
        y = quant.matmul_hadU_cuda(torch.from_numpy(x).to(DEV), hd, K, n, transpose=True)
        ref = O.matmul_hadU(x.astype(np.float64), None if had is None else had.astype(np.float64), K, n, transpose=True)
        err = np.abs(y.cpu().numpy().astype(np.float64) - ref)
        bound = 2.0 ** -10 * np.abs(ref) + 2.0 ** -18 * np.linalg.norm(ref, axis=1, keepdims=True) + 1e-6
        print("fp16 n=%d K=%d: max err / bound %.3f" % (n, K, (err / bound).max()))
        assert np.all(err <= bound)
        return
    scale = 0.37 / np.sqrt(n // K)
    p = torch.ops.quip_lib.had_transform_planes(torch.from_numpy(x).to(DEV), n, K, hd, True, torch.from_numpy(su).to(DEV),
                                                float(scale))
    X, sh, kp = _decode_planes(p, n)
    assert np.all(np.abs(X) < 2 ** 22) and np.all(X[n:] == 0)
    ref = O.matmul_hadU(x.astype(np.float64) * su.astype(np.float64), None if had is None else had.astype(np.float64), K, n,
                        scale=0.37, transpose=True)[0]
    got = X[:n].astype(np.float64) * 2.0 ** -sh
    tol = 2.0 ** (-sh - 1) + 2.0 ** -20 * np.linalg.norm(ref) / np.sqrt(n) * np.log2(n) + 1e-9
    print("planes n=%d K=%d: max err / bound %.3f" % (n, K, np.max(np.abs(got - ref)) / (tol * 1.5)))
    assert np.max(np.abs(got - ref)) <= tol * 1.5


@pytest.mark.parametrize("planes", [False, True], ids=["fp16", "planes"])
def test_lds_limit_survives_a_smaller_request_from_another_call_site(Q, planes):
    """had_fast_kernel<planes, false, 1024> has two call sites in csrc/hadamard.hip: the long K == 1 row (n = 16384: 2 *
    buf_floats(16384) * 4 = 135 200 bytes of LDS) and the K > 1 row split over thread groups (n = 28672 = 7 x 4096: 82 976
    bytes).  Both sizes lie above the 48 KB a kernel gets without hipFuncAttributeMaxDynamicSharedMemorySize.  With one
    launch state per kernel the smaller request in between never lowers the limit under the larger one."""
    from quip_for_all_amd.quant import get_hadK
    np.random.seed(28672)                      # (get_hadK draws its rotation from numpy's global state)
    had7, K7, _ = get_hadK(28672)              # the library's own 7 x 7 factor
    assert K7 == 7
    had7 = had7.numpy().astype(np.float16)
    rng = np.random.default_rng(16384 + planes)
    big = rng.standard_normal((1, 16384)).astype(np.float16)
    su_big = (rng.integers(0, 2, 16384) * 2 - 1).astype(np.float16)
    mid = rng.standard_normal((1, 28672)).astype(np.float16)
    su_mid = (rng.integers(0, 2, 28672) * 2 - 1).astype(np.float16)
    _transform(planes, big, su_big, None, 16384, 1)
    _transform(planes, mid, su_mid, had7, 28672, 7)
    _transform(planes, big, su_big, None, 16384, 1)
    torch.cuda.synchronize()


def _check_mm(y, x, W64):
    x64 = x.cpu().numpy().astype(np.float64)
    y64 = x64 @ W64.T
    err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
    assert np.all(err <= _mm_tol(x64, W64, y64)), err.max()


@pytest.mark.parametrize("m", [1, 17])
def test_skinny_launch(Q, m):
    """e8p_skinny_gemm_kernel<1, 16> / <1, 32> (m <= 16 / m > 16), n = 64, k = 128"""
    n, k = 64, 128
    P = O.make_layer("E8P12", k, n, seed=m)
    x = torch.from_numpy(np.random.default_rng(m).standard_normal((m, k)).astype(np.float16)).to(DEV)
    y = torch.ops.quip_lib.e8p_mm_skinny(x, torch.from_numpy(P.Qidxs).to(DEV), _cb(Q, "E8P12").grid_packed_abs)
    assert y.shape == (m, n)
    _check_mm(y, x, O.decompress_e8p(P.Qidxs).astype(np.float64))


@pytest.mark.parametrize("cbid", ["E8P12", "E8P12RVQ3B"], ids=["mode0", "mode4"])
def test_tile_gemm_launch(Q, cbid):
    """e8p_prefill_gemm_kernel in mode 0 (E8P12) and mode 4 (E8P12RVQ3B: the third table), m = 32, n = 64, k = 128"""
    from quip_for_all_amd.qlinear import QuantLinear
    m, n, k = 32, 64, 128
    P = O.make_layer(cbid, k, n, seed=5)
    layer = QuantLinear.from_params(P).to(DEV).eval()
    assert (layer.q_in_features, layer.q_out_features) == (k, n)
    x = torch.from_numpy(np.random.default_rng(6).standard_normal((m, k)).astype(np.float16)).to(DEV)
    cb = layer.codebook
    y = torch.ops.quip_lib.e8p_mm_batched(x, layer.Qidxs, cb.grid_packed_abs) if cbid == "E8P12" else cb.mm_batched(x, layer.Qidxs)
    assert y.shape == (m, n)
    _check_mm(y, x, O.decompress(cbid, P.Qidxs, getattr(layer.codebook, "opt_resid_scale", 0.0)).astype(np.float64))


def test_tile_then_untile_round_trip(Q):
    from quip_for_all_amd import capi
    L = capi.lib()
    st = torch.cuda.current_stream().cuda_stream
    src = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (16, 64), dtype=np.uint8)).to(DEV)
    tiled, back = torch.zeros_like(src), torch.zeros_like(src)
    assert L.quip_tile_codes(src.data_ptr(), tiled.data_ptr(), 16, 64, st) == 0
    assert L.quip_untile_codes(tiled.data_ptr(), back.data_ptr(), 16, 64, st) == 0
    assert torch.equal(back, src)
    # tiled[c][q][n] = bytes [16 q, +16) of row n (one row block, one 64-byte piece)
    assert torch.equal(tiled.view(4, 16, 16), src.view(16, 4, 16).transpose(0, 1))


def test_k_split_gemv_forced_split_byte_and_nibble_mode(Q):
    """n = 8, k = 2048, K split 2: e8p_gemv_v2_kernel and e8p_gemv_v2n_kernel give the first kernel's bits"""
    n, k = 8, 2048
    L, P, x, Qd, planes, st = _setup(Q, n, k, seed=n + k)
    grid = _cb(Q, "E8P12").grid_packed_abs
    ws = torch.zeros(L.quip_e8p_gemv_v2_workspace_bytes(n) // 4, dtype=torch.int32, device=DEV)
    ys = {}
    for rep in (32, 4):
        ys[rep] = torch.full((1, n), float("nan"), dtype=torch.float16, device=DEV)
        assert L.quip_e8p_gemv_v2_tuned(planes.data_ptr(), Qd.data_ptr(), grid.data_ptr(), ys[rep].data_ptr(), ws.data_ptr(),
                                        n, k, rep, 0, 0, 2, 0, 0, None, st) == 0
        assert int(ws.abs().max()) == 0, "workspace must be left zeroed"
    y1 = torch.empty_like(ys[4])
    assert L.quip_e8p_gemv_tuned(planes.data_ptr(), Qd.data_ptr(), grid.data_ptr(), y1.data_ptr(), n, k, 4, 0, 0, 0, 0, 0, 0,
                                 None, st) == 0
    assert torch.equal(ys[32].view(torch.int16), ys[4].view(torch.int16))
    assert torch.equal(ys[32].view(torch.int16), y1.view(torch.int16))
    _check_mm(ys[32], x, O.decompress_e8p(P.Qidxs).astype(np.float64))
    from quip_for_all_amd import capi
    assert capi.gemv_v2_plan([n], k, 32, ksplit=2)[3] == 2 and capi.gemv_v2_plan([n], k, 4, ksplit=2)[3] == 2
