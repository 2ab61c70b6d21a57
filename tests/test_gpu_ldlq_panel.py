"""quip_lib::ldlq_panel (csrc/quantize.hip) and quant.LDLQ on it: every rounding step of the fused route against a float64
recomputation of its target, the tune sweep, both routes on the reference's goldens, row independence, the shared search
and the operand checks."""
import os

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from quip_for_all_amd import quant

from tests import ldlq_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize_golden.npz"))
_RESULTS = {}


def _cb():
    import quip_for_all_amd as Q
    return Q.codebook.codebook_id["E8P12"](inference=False).to(DEV)


def _fused(m, n, iters):
    """LDLQ on the fused route, once per (shape, iters): (W, H, L64, hat, Qidxs) as numpy"""
    key = (m, n, iters)
    if key not in _RESULTS:
        W, H = C.make_case(m, n)
        L64 = C.chol64(H)
        Wt, Ht, Lt = (torch.from_numpy(a).to(DEV) for a in (W, H, L64.astype(np.float32)))
        assert quant.ldlq_route(Wt, _cb()) == "panels"
        hat, Q = quant.LDLQ(Wt.clone(), Ht.clone(), Lt.clone(), _cb(), iters)
        _RESULTS[key] = (W, H, L64, hat.cpu().numpy(), Q.cpu().numpy())
    return _RESULTS[key]


@pytest.mark.parametrize("m,n", C.SHAPES)
def test_every_step_is_consistent_with_float64(m, n):
    """For every group k of every row, the target recomputed in float64 from W, the block-LDL factor of the float64 Cholesky
    and the kernel's own hat right of k: the codeword the kernel chose is a nearest one up to the fp32 accumulation bound of
    that target (tests/ldlq_cases.check_ldlq_steps).  No exceptions."""
    W, H, L64, hat, Q = _fused(m, n, 0)
    over, steps, worst = C.check_ldlq_steps(W, O.block_ldl(L64, 8), hat)
    print(f"ldlq_panel ({m}, {n}): {over} of {steps} steps over the bound, largest excess over the nearest point {worst:.3e}")
    assert steps == m * (n // 8) and over == 0
    dec = O.e8p_decode_i8(Q.astype(np.uint16)).astype(np.float32) / 4            # (m, n / 8, 8)
    assert np.array_equal(hat, dec.reshape(m, n))


@pytest.mark.parametrize("m,n", C.SHAPES)
def test_tune_sweep(m, n):
    W, H, L64, hat0, _ = _fused(m, n, 0)
    _, _, _, hat1, Q1 = _fused(m, n, 1)
    over, steps, worst = C.check_tune_steps(W, H, hat0, hat1)
    print(f"tune sweep ({m}, {n}): {over} of {steps} steps over the bound, largest excess {worst:.3e}")
    assert over == 0
    assert np.array_equal(hat1, (O.e8p_decode_i8(Q1.astype(np.uint16)).astype(np.float32) / 4).reshape(m, n))
    # the sweep may not raise the proxy loss by more than the stepwise route's sweep does on the same input
    Wt, Ht, Lt = (torch.from_numpy(a).to(DEV) for a in (W, H, L64.astype(np.float32)))
    s0, _ = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), _cb(), 0)
    s1, _ = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), _cb(), 1)
    rise_fused = C.proxy_loss(W, hat1, H) - C.proxy_loss(W, hat0, H)
    rise_step = C.proxy_loss(W, s1.cpu().numpy(), H) - C.proxy_loss(W, s0.cpu().numpy(), H)
    print(f"proxy loss change of one sweep: fused {rise_fused:.6e}, stepwise {rise_step:.6e}")
    assert max(rise_fused, 0.0) <= max(rise_step, 0.0)


@pytest.mark.parametrize("iters", [0, 1])
@pytest.mark.parametrize("route", ["panels", "stepwise"])
def test_routes_agree_with_the_reference_goldens(route, iters, monkeypatch):
    """tests/test_gpu_quantize.py::test_ldlq_matches_reference's own criteria, on the fused route called explicitly and on
    LDLQ with QUIP_LDLQ_FUSED=0"""
    cb = _cb()
    W = torch.from_numpy(G["ldlq_E8P12_W"]).to(DEV)
    H = torch.from_numpy(G["ldlq_E8P12_H"]).to(DEV)
    L = torch.linalg.cholesky(H)
    if route == "stepwise":
        monkeypatch.setattr(quant, "_LDLQ_FUSED", None)
        monkeypatch.setenv("QUIP_LDLQ_FUSED", "0")
        assert quant.ldlq_route(W, cb) == "stepwise"
        run = quant.LDLQ
    else:
        run = quant.LDLQ_panels
    Wn, Hn = G["ldlq_E8P12_W"].astype(np.float64), G["ldlq_E8P12_H"].astype(np.float64)
    e_ref = C.proxy_loss(Wn, G[f"ldlq_E8P12_{iters}_hatW"], Hn)
    ref = G[f"ldlq_E8P12_{iters}_Qidxs"].astype(np.int64) & 0xffff
    for buf in (128, 16):
        hat, Q = run(W.clone(), H.clone(), L.clone(), cb, iters, buf_cols=buf)
        got = Q.cpu().numpy().astype(np.int64) & 0xffff
        assert (got == ref).mean() >= 0.98, (route, buf, (got == ref).mean())
        e_got = C.proxy_loss(Wn, hat.cpu().numpy(), Hn)
        assert abs(e_got - e_ref) <= 0.02 * e_ref, (route, buf, e_got, e_ref)


def _operands(m, c, with_p, seed=0):
    g = torch.Generator().manual_seed(100 * c + m + seed)
    A = torch.randn(m, c, generator=g) * 1.1
    B = torch.randn(m, c, generator=g) * 0.2
    M = torch.randn(c, c, generator=g) * 0.1
    P = (torch.eye(8) + 0.1 * torch.randn(c // 8, 8, 8, generator=g)) if with_p else None
    return A.to(DEV), B.to(DEV), M.to(DEV), None if P is None else P.contiguous().to(DEV)


@pytest.mark.parametrize("c,with_p", [(128, False), (128, True), (48, True), (8, False)])
def test_rows_are_independent_and_runs_repeat(c, with_p):
    cb = _cb()
    A, B, M, P = _operands(40, c, with_p)
    hat, idx = torch.ops.quip_lib.ldlq_panel(A, B, M, P, cb.grid_packed_abs)
    assert tuple(hat.shape) == (40, c) and tuple(idx.shape) == (40, c // 8) and idx.dtype == torch.int64
    hat2, idx2 = torch.ops.quip_lib.ldlq_panel(A, B, M, P, cb.grid_packed_abs)
    assert torch.equal(hat, hat2) and torch.equal(idx, idx2)
    parts = [torch.ops.quip_lib.ldlq_panel(A[r].contiguous(), B[r].contiguous(), M, P, cb.grid_packed_abs)
             for r in (slice(0, 7), slice(7, 40))]
    assert torch.equal(hat, torch.cat([p[0] for p in parts])) and torch.equal(idx, torch.cat([p[1] for p in parts]))
    # the recursion itself, in float64 on the kernel's own hat: with M and P in play the target differs from A + B
    Ad, Bd, Md, hd = (t.double().cpu() for t in (A, B, M, hat))
    E = Ad - hd
    k = 0
    t = Bd[:, :8] + E[:, 8:] @ Md[8:, :8]
    t = Ad[:, :8] + (t @ P[k].double().cpu() if with_p else t)
    vals, _ = O.quantize("E8P12", t.numpy())
    d = np.linalg.norm(t.numpy() - hd[:, :8].numpy(), axis=1)
    dstar = np.linalg.norm(t.numpy() - vals, axis=1)
    inner = np.abs(Bd[:, :8]) + np.abs(E[:, 8:]) @ np.abs(Md[8:, :8])
    scale = np.abs(Ad[:, :8]) + (inner @ P[k].double().abs().cpu() if with_p else inner)
    eps = (c + 10) * C.U32 * np.linalg.norm(scale.numpy(), axis=1)      # c - 8 + 8 products and three additions, each u
    assert np.all(d <= dstar + 2 * eps)


@pytest.mark.parametrize("m,c", [(40, 128), (33, 48), (5, 8), (1, 16)])
def test_same_search_as_e8p_quantize(m, c):
    """M = 0 and no P: every group's target is A + B, and the codeword is the one e8p_quantize gives for it, bit for bit"""
    cb = _cb()
    A, B, _, _ = _operands(m, c, False, seed=3)
    A[0] = 0.0
    B[0] = 0.0                                                          # ties at the origin too
    hat, idx = torch.ops.quip_lib.ldlq_panel(A, B, torch.zeros(c, c, device=DEV), None, cb.grid_packed_abs)
    vals, ix = torch.ops.quip_lib.e8p_quantize((A + B).reshape(-1, 8).contiguous(), cb.grid_packed_abs)
    assert torch.equal(idx, ix.reshape(m, c // 8)) and torch.equal(hat, vals.reshape(m, c))


def test_operand_checks():
    cb = _cb()
    g = cb.grid_packed_abs
    A, B, M, P = _operands(8, 16, True)
    op = torch.ops.quip_lib.ldlq_panel
    op(A, B, M, P, g)
    bad = [
        (A.double(), B, M, P, g), (A, B.half(), M, P, g), (A, B, M.double(), P, g), (A, B, M, P.half(), g),   # dtype
        (A.t().contiguous().t(), B, M, P, g), (A, B, M.t(), P, g), (A, B, M, P.transpose(1, 2), g),           # contiguity
        (A[:, :12].contiguous(), B[:, :12].contiguous(), M[:12, :12].contiguous(), None, g),                  # c % 8
        (A, B[:4].contiguous(), M, P, g), (A, B, M[:8].contiguous(), P, g), (A, B, M, P[:1].contiguous(), g),  # shapes
        (A, B, M, torch.zeros(2, 8, 4, device=DEV), g),
        (A, B, M, P, g[:128].contiguous()), (A, B.cpu(), M, P, g), (A, B, M, P, g.to(torch.int32)),           # table, device
    ]
    wide = _operands(4, 136, False)
    bad.append((wide[0], wide[1], wide[2], None, g))                                                           # c > 128
    for args in bad:
        with pytest.raises((ValueError, RuntimeError)):
            op(*args)
    torch.cuda.synchronize()
