"""The stand-alone GEMV entry points of the C ABI that no op and no other GPU test calls -- quip_e8p_gemv_planes_ws,
quip_e8p_gemv_planes_rows, quip_d4_gemv_planes, quip_d4_gemv_planes_group and quip_e8prvq3_gemv_planes_group (quip_e8p_gemv_planes runs in
test_gpu_gemv_v2, quip_d4_gemv_planes_v2 in test_gpu_qlinear) -- through ctypes, each at the smallest shape the GEMV tests
use for its table mode: bit for bit what the group op with a workspace gives on the same planes and codes.  The sums are
integer sums, so which kernel and which plan a launch takes does not show in the bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_gpu_ops import DEV, _cb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def Q():
    assert torch.cuda.is_available()
    import quip_for_all_amd as Q
    return Q


def _planes(L, digits, seed):
    """the digit planes of a random fp16 vector of `digits` elements"""
    x = torch.from_numpy(np.random.default_rng(seed).standard_normal((1, digits)).astype(np.float16)).to(DEV)
    planes = torch.empty(L.quip_e8p_planes_bytes(digits), dtype=torch.uint8, device=DEV)
    assert L.quip_e8p_x_to_planes(x.data_ptr(), planes.data_ptr(), digits, torch.cuda.current_stream().cuda_stream) == 0
    return planes


def _codes(shape, dtype, seed):
    info = np.iinfo(dtype)
    return torch.from_numpy(np.random.default_rng(seed).integers(info.min, info.max, size=shape, endpoint=True, dtype=dtype)).to(DEV)


def _group_args(planes, codes):
    vp = ctypes.c_void_p * len(codes)
    ys = [torch.full((1, q.shape[0]), float("nan"), dtype=torch.float16, device=DEV) for q in codes]
    ns = (ctypes.c_int32 * len(codes))(*[q.shape[0] for q in codes])
    return ys, vp(*[p.data_ptr() for p in planes]), vp(*[q.data_ptr() for q in codes]), vp(*[y.data_ptr() for y in ys]), ns


def test_e8p_single_matrix_with_a_workspace(Q):
    L, (n, k) = Q.capi.lib(), (4, 128)
    cb = _cb(Q, "E8P12")
    planes, q = _planes(L, k, 1), _codes((n, k // 8), np.int16, 2)
    ws = torch.zeros(L.quip_e8p_gemv_workspace_bytes(n) // 4, dtype=torch.int32, device=DEV)
    y = torch.full((1, n), float("nan"), dtype=torch.float16, device=DEV)
    Q.capi.check(L.quip_e8p_gemv_planes_ws(planes.data_ptr(), q.data_ptr(), cb.grid_packed_abs.data_ptr(), y.data_ptr(), n, k,
                                           ws.data_ptr(), ws.numel() * 4, torch.cuda.current_stream().cuda_stream),
                 "quip_e8p_gemv_planes_ws")
    (ref,) = torch.ops.quip_lib.e8p_gemv_planes_group([planes], [q], cb.grid_packed_abs)
    assert torch.equal(y, ref) and not ws.any()                     # (a launch leaves its workspace zeroed)


def test_e8p_rows_entry_is_rows_mode_0(Q):
    """quip_e8p_gemv_planes_rows (the rows op goes through quip_gemv_planes_rows_mode, which this entry forwards to) at the
    smallest shape of test_gpu_ops' rows test, all five rows in one pass"""
    L, (n, k, M) = Q.capi.lib(), (48, 1024, 5)
    cb = _cb(Q, "E8P12")
    assert L.quip_e8p_gemv_max_rows(n, k) >= M
    planes = torch.stack([_planes(L, k, 20 + r) for r in range(M)])
    q = _codes((n, k // 8), np.int16, 9)
    y = torch.full((M, n), float("nan"), dtype=torch.float16, device=DEV)
    Q.capi.check(L.quip_e8p_gemv_planes_rows(planes.data_ptr(), q.data_ptr(), cb.grid_packed_abs.data_ptr(), y.data_ptr(), M, n, k,
                                             torch.cuda.current_stream().cuda_stream), "quip_e8p_gemv_planes_rows")
    assert torch.equal(y, torch.ops.quip_lib.e8p_gemv_planes_rows(planes, q, cb.grid_packed_abs))


def test_d4_single_matrix_and_group_of_two(Q):
    L, (n, k) = Q.capi.lib(), (1000, 256)
    cb = _cb(Q, "D4")
    st = torch.cuda.current_stream().cuda_stream
    planes = [_planes(L, k, 3), _planes(L, k, 4)]
    codes = [_codes((n, k // 4), np.uint8, 5), _codes((n, k // 4), np.uint8, 6)]
    ref = torch.ops.quip_lib.d4_gemv_planes_group(planes, codes, cb.grid)
    y = torch.full((1, n), float("nan"), dtype=torch.float16, device=DEV)
    Q.capi.check(L.quip_d4_gemv_planes(planes[0].data_ptr(), codes[0].data_ptr(), cb.grid.data_ptr(), y.data_ptr(), n, k, st),
                 "quip_d4_gemv_planes")
    assert torch.equal(y, ref[0])
    ys, pp, qp, yp, ns = _group_args(planes, codes)
    Q.capi.check(L.quip_d4_gemv_planes_group(pp, qp, cb.grid.data_ptr(), yp, ns, 2, k, st), "quip_d4_gemv_planes_group")
    assert torch.equal(ys[0], ref[0]) and torch.equal(ys[1], ref[1])


def test_e8prvq3_group_of_two(Q):
    L, k, fouts = Q.capi.lib(), 256, (256, 688)
    cb = _cb(Q, "E8P12RVQ3B", 1 / 2.04)
    planes = [_planes(L, 2 * k, 7)] * 2                             # (the virtual vector: 2 k digits)
    codes = [_codes((n, 3 * k // 32), np.int32, 8 + i) for i, n in enumerate(fouts)]
    e81b = cb._e81b_i8(torch.device(DEV))
    ref = torch.ops.quip_lib.e8prvq3_gemv_planes_group(planes, codes, cb.grid_packed_abs, e81b)
    ys, pp, qp, yp, ns = _group_args(planes, codes)
    Q.capi.check(L.quip_e8prvq3_gemv_planes_group(pp, qp, cb.grid_packed_abs.data_ptr(), e81b.data_ptr(), yp, ns, 2, k,
                                                  torch.cuda.current_stream().cuda_stream), "quip_e8prvq3_gemv_planes_group")
    assert torch.equal(ys[0], ref[0]) and torch.equal(ys[1], ref[1])
