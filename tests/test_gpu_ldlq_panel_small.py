"""quip_lib::ldlq_panel_small (csrc/ldlq_panel_small.hip) and quant.LDLQ on it for D4 / HI behind QUIP_LDLQ_FUSED_SMALL: the
recursion bit for bit on exact operands, the rounding alone, row independence, every step of LDLQ and of a tune sweep
against float64, the criteria the stepwise route is held to, and the operand checks."""
import os

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from quip_for_all_amd import quant

from tests import ldlq_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CBIDS = ["D4", "HI"]
CODESZ = {"D4": 4, "HI": 1}
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize_golden.npz"))
_RUNS = {}


def _cb(cbid):
    import quip_for_all_amd as Q
    return Q.codebook.codebook_id[cbid](inference=False).to(DEV)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _op(cbid, A, B, M, P):
    grid = _dev(O.d4_grid()) if cbid == "D4" else None
    hat, idx = torch.ops.quip_lib.ldlq_panel_small(_dev(A), _dev(B), _dev(M), _dev(P), grid)
    return hat.cpu().numpy(), idx.cpu().numpy()


def _decode(cbid, idx):
    return (O.d4_grid()[idx].reshape(idx.shape[0], -1) if cbid == "D4" else idx - 7.5).astype(np.float32)


def _dyadic(cbid, m, c, with_p):
    """operands on which every product and partial sum of the recursion is exact in fp32; row 0 all zeros (ties: the lowest
    index wins), row 1 on midpoints between levels (integers)"""
    b, amp = CODESZ[cbid], 10 if cbid == "HI" else 4
    rng = np.random.default_rng(100 * c + m + with_p)
    A, B = (rng.integers(-8 * amp, 8 * amp + 1, (m, c)) / 8.0 for _ in range(2))
    M = rng.integers(-8, 9, (c, c)) / 8.0
    P = np.eye(b) + rng.integers(-2, 3, (c // b, b, b)) / 4.0 if with_p else None
    if m > 1:
        A[0] = B[0] = B[1] = 0.0
        A[1] = np.round(A[1] / 2)
    return A, B, M, P


@pytest.mark.parametrize("lanes", [8, 16])
@pytest.mark.parametrize("with_p", [False, True])
@pytest.mark.parametrize("m,c", [(1, 0), (33, 48), (40, 128), (5, 8)])      # c = 0: a single group, c = b
@pytest.mark.parametrize("cbid", CBIDS)
def test_exact_recursion_on_dyadic_operands(cbid, m, c, with_p, lanes, monkeypatch):
    """hat and idx equal the recursion in float64 with oracle.quantize as the search, for both instantiations"""
    monkeypatch.setenv("QUIP_LDLQ_SMALL_LANES", str(lanes))
    b = CODESZ[cbid]
    A, B, M, P = _dyadic(cbid, m, c or b, with_p)
    hat, idx = _op(cbid, A, B, M, P)
    want = np.zeros_like(A)
    for k in range(A.shape[1] // b - 1, -1, -1):      # the recursion in float64 with the oracle as the search
        lo, hi = k * b, k * b + b
        t = B[:, lo:hi] + (A[:, hi:] - want[:, hi:]) @ M[hi:, lo:hi]
        want[:, lo:hi], want_idx = O.quantize(cbid, A[:, lo:hi] + (t if P is None else t @ P[k]))
        assert np.array_equal(idx[:, k], want_idx), k
    assert np.array_equal(hat, want)


@pytest.mark.parametrize("cbid", CBIDS)
def test_rounding_alone(cbid):
    """M = 0, no P: every group's target is fl(A + B); the codeword is nearest in float64 up to the fp32 rounding of the score
    (D4: four products, three sums, the doubling's subtraction -- 6 u (|t| + 1) per coordinate); HI has no rounding at all"""
    b = CODESZ[cbid]
    rng = np.random.default_rng(5)
    A, B = (rng.standard_normal((40, 128)).astype(np.float32) * s for s in (2.0 if cbid == "D4" else 6.0, 0.3))
    hat, idx = _op(cbid, A, B, np.zeros((128, 128)), None)
    t = (A + B).astype(np.float64).reshape(-1, b)
    best, best_idx = O.quantize(cbid, t)
    assert np.array_equal(hat, _decode(cbid, idx))
    if cbid == "HI":
        assert np.array_equal(idx.reshape(-1), best_idx)
    d, dstar = np.linalg.norm(t - hat.reshape(-1, b), axis=1), np.linalg.norm(t - best, axis=1)
    assert np.all(d <= dstar + 2 * 6 * C.U32 * np.linalg.norm(np.abs(t) + 1, axis=1))


@pytest.mark.parametrize("cbid", CBIDS)
def test_rows_are_independent_and_runs_repeat(cbid, monkeypatch):
    """... and a row's bits do not depend on the lanes per row (random operands: the summation order is the same)"""
    b = CODESZ[cbid]
    rng = np.random.default_rng(9)
    A, B, M = rng.standard_normal((40, 128)) * 1.5, rng.standard_normal((40, 128)) * 0.2, rng.standard_normal((128, 128)) * 0.1
    P = np.eye(b) + 0.1 * rng.standard_normal((128 // b, b, b))
    hat, idx = _op(cbid, A, B, M, P)
    again = _op(cbid, A, B, M, P)
    assert np.array_equal(hat, again[0]) and np.array_equal(idx, again[1])
    parts = [_op(cbid, A[r], B[r], M, P) for r in (slice(0, 7), slice(7, 40))]
    monkeypatch.setenv("QUIP_LDLQ_SMALL_LANES", "16")
    parts.append(_op(cbid, A, B, M, P))
    assert np.array_equal(hat, np.concatenate([p[0] for p in parts[:2]])) and np.array_equal(hat, parts[2][0])
    assert np.array_equal(idx, np.concatenate([p[1] for p in parts[:2]])) and np.array_equal(idx, parts[2][1])


def _ldlq(cbid, m, n, iters, monkeypatch, run=None):
    """quant.LDLQ with the switch on (or `run`), once per case: (W, H, L64, hat, Q) as numpy"""
    key = (cbid, m, n, iters, run)
    if key not in _RUNS:
        monkeypatch.setattr(quant, "_LDLQ_FUSED", True)
        monkeypatch.setattr(quant, "_LDLQ_FUSED_SMALL", None)
        monkeypatch.setenv("QUIP_LDLQ_FUSED_SMALL", "1")
        W, H = C.make_case(m, n)
        L64 = C.chol64(H)
        Wt, Ht, Lt = (torch.from_numpy(a).to(DEV) for a in (W, H, L64.astype(np.float32)))
        assert quant.ldlq_route(Wt, _cb(cbid)) == "panels"
        hat, Q = (run or quant.LDLQ)(Wt.clone(), Ht.clone(), Lt.clone(), _cb(cbid), iters)
        _RUNS[key] = (W, H, L64, hat.cpu().numpy(), Q.cpu().numpy().astype(np.int64))
    return _RUNS[key]


def _steps_over(cbid, W, hat, Lb=None, H=None, hb=None):
    """tests/ldlq_cases.check_ldlq_steps (Lb given) / check_tune_steps (H and the pre-sweep hat given) over groups of b columns:
    the steps whose codeword is further from the float64 target than the float64 nearest one by more than 2 eps_k,
    eps_k = (n - hi + 2) u || |W_k| + |E| |Lb_{>k,k}| ||   /   (n + b + 2) u || |hb_k| + (|W - mixed| |H[:, k]|) |inv(H_kk)| ||"""
    b, n = CODESZ[cbid], W.shape[1]
    W, hat = W.astype(np.float64), hat.astype(np.float64)
    over = 0
    for lo in range(n - b, -1, -b):
        hi = lo + b
        if Lb is not None:
            E = W[:, hi:] - hat[:, hi:]
            t = W[:, lo:hi] + E @ Lb[hi:, lo:hi]
            eps = (n - hi + 2) * C.U32 * np.linalg.norm(np.abs(W[:, lo:hi]) + np.abs(E) @ np.abs(Lb[hi:, lo:hi]), axis=1)
        else:
            D, Pk = W - np.concatenate([hb[:, :hi], hat[:, hi:]], axis=1), np.linalg.inv(H[lo:hi, lo:hi].astype(np.float64))
            t = hb[:, lo:hi] + D @ H[:, lo:hi] @ Pk
            eps = (n + b + 2) * C.U32 * np.linalg.norm(np.abs(hb[:, lo:hi]) + np.abs(D) @ np.abs(H[:, lo:hi]) @ np.abs(Pk), axis=1)
        gstar, _ = O.quantize(cbid, t)
        over += int((np.linalg.norm(t - hat[:, lo:hi], axis=1) > np.linalg.norm(t - gstar, axis=1) + 2.0 * eps).sum())
    return over


@pytest.mark.parametrize("m,n", C.SHAPES)
@pytest.mark.parametrize("cbid", CBIDS)
def test_every_ldlq_and_tune_step_is_consistent_with_float64(cbid, m, n, monkeypatch):
    W, H, L64, hat0, Q0 = _ldlq(cbid, m, n, 0, monkeypatch)
    assert _steps_over(cbid, W, hat0, Lb=O.block_ldl(L64, CODESZ[cbid])) == 0
    assert np.array_equal(hat0, _decode(cbid, Q0))
    _, _, _, hat1, Q1 = _ldlq(cbid, m, n, 1, monkeypatch)
    assert _steps_over(cbid, W, hat1, H=H.astype(np.float64), hb=hat0.astype(np.float64)) == 0
    assert np.array_equal(hat1, _decode(cbid, Q1))


@pytest.mark.parametrize("iters", [0, 1])
@pytest.mark.parametrize("cbid", CBIDS)
def test_what_the_stepwise_route_is_held_to(cbid, iters, monkeypatch):
    """D4: tests/test_gpu_quantize.py::test_ldlq_matches_reference's criteria on the reference goldens; HI (no golden): the proxy
    loss within the same 2 % of LDLQ_stepwise's on make_case(24, 64)"""
    if cbid == "HI":
        W, H, _, hat, _ = _ldlq(cbid, 24, 64, iters, monkeypatch)
        e_ref = C.proxy_loss(W, _ldlq(cbid, 24, 64, iters, monkeypatch, run=quant.LDLQ_stepwise)[3], H)
        assert abs(C.proxy_loss(W, hat, H) - e_ref) <= 0.02 * e_ref
        return
    Wn, Hn = G["ldlq_D4_W"], G["ldlq_D4_H"]
    W, H = torch.from_numpy(Wn).to(DEV), torch.from_numpy(Hn).to(DEV)
    L = torch.linalg.cholesky(H)
    e_ref = C.proxy_loss(Wn, G[f"ldlq_D4_{iters}_hatW"], Hn)
    for buf in (128, 16):
        hat, Q = quant.LDLQ_panels_small(W.clone(), H.clone(), L.clone(), _cb(cbid), iters, buf_cols=buf)
        same = (Q.cpu().numpy().astype(np.int64) & 0xff) == (G[f"ldlq_D4_{iters}_Qidxs"].astype(np.int64) & 0xff)
        assert same.mean() >= 0.98, (buf, same.mean())
        assert abs(C.proxy_loss(Wn, hat.cpu().numpy(), Hn) - e_ref) <= 0.02 * e_ref, buf


def test_operand_checks():
    op = torch.ops.quip_lib.ldlq_panel_small
    A, B, M = (torch.randn(s, device=DEV) for s in ((8, 16), (8, 16), (16, 16)))
    P, P1, g = torch.randn(4, 4, 4, device=DEV), torch.randn(16, 1, 1, device=DEV), _dev(O.d4_grid())
    assert tuple(op(A, B, M, P, g)[1].shape) == (8, 4)
    assert tuple(op(A, B, M, P1, None)[1].shape) == (8, 16)                  # no table and c % 4 == 0: HI
    six, wide = (torch.randn(4, 6, device=DEV), torch.randn(6, 6, device=DEV)), torch.randn(4, 136, device=DEV)
    bad = [(A.double(), B, M, P, g), (A, B.half(), M, P, g), (A, B, M, P.half(), g),                 # dtype
           (A.t().contiguous().t(), B, M, P, g), (A, B, M.t(), P, g), (A, B, M, P.transpose(1, 2), g),   # contiguity
           (six[0], six[0], six[1], None, g),                                                         # c % 4
           (wide, wide, torch.zeros(136, 136, device=DEV), None, g), (wide, wide, torch.zeros(136, 136, device=DEV), None, None),
           (A, B, M, torch.zeros(2, 8, 8, device=DEV), g), (A, B, M, torch.zeros(2, 8, 8, device=DEV), None),   # the 8-wide P
           (A, B, M, P, None), (A, B, M, P1, g), (A, B[:4].contiguous(), M, P, g), (A, B, M[:8].contiguous(), P, g),
           (A, B, M, P, g[:128].contiguous()), (A, B, M, P, g.reshape(4, 256)), (A, B, M, P, g.cpu()), (A, B, M, P, g.half())]
    for args in bad:
        with pytest.raises((ValueError, RuntimeError)):
            op(*args)
    assert tuple(op(A, B, M, P, g)[0].shape) == (8, 16)
    torch.cuda.synchronize()
