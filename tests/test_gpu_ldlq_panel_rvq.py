"""quip_lib::ldlq_panel_rvq (csrc/quantize.hip) and quant.LDLQ_panels on it for E8P12RVQ4B / E8P12RVQ3B: both stages of every
rounding step of the fused route against a float64 recomputation of its target, the tune sweep, both routes against the float64
oracle, the written-out stepwise chain bit for bit, row independence, a non-default scale, the operand checks, and the route
through QUIP.quant behind QUIP_LDLQ_FUSED_RVQ."""
import os

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from quip_for_all_amd import quant

from tests import ldlq_cases as C
from tests import ldlq_rvq_cases as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "quantize_golden.npz"))
_RESULTS, _ORACLE = {}, {}


def _cb(cbid, **kw):
    import quip_for_all_amd as Q
    return Q.codebook.codebook_id[cbid](inference=False, **kw).to(DEV)


def _op(cb, A, B, M, P, scale=None):
    resid = cb.e81b_grid.to(torch.float32).contiguous() if cb.id == "E8P12RVQ3B" else None
    s = cb.opt_resid_scale if scale is None else scale
    return torch.ops.quip_lib.ldlq_panel_rvq(A, B, M, P, cb.grid_packed_abs, resid, s)


def _fused(cbid, m, n, iters):
    """LDLQ on the fused route, once per (codebook, shape, iters): (W, H, L64, hat, Qidxs) as numpy"""
    key = (cbid, m, n, iters)
    if key not in _RESULTS:
        W, H = C.make_case(m, n)
        L64 = C.chol64(H)
        Wt, Ht, Lt = (torch.from_numpy(a).to(DEV) for a in (W, H, L64.astype(np.float32)))
        hat, Q = quant.LDLQ_panels(Wt.clone(), Ht.clone(), Lt.clone(), _cb(cbid), iters)
        assert Q.dtype == torch.int32
        _RESULTS[key] = (W, H, L64, hat.cpu().numpy(), Q.cpu().numpy())
    return _RESULTS[key]


@pytest.mark.parametrize("m,n", C.SHAPES)
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_every_step_is_consistent_with_float64(cbid, m, n):
    """tests/ldlq_rvq_cases.check_rvq_steps on the kernel's own hat and indices: for every group of every row both stage
    points are nearest ones of their float64 targets up to the fp32 accumulation bound, and hat is the fp32 decode of the
    stored codes.  No exceptions."""
    W, H, L64, hat, Q = _fused(cbid, m, n, 0)
    rep = R.check_rvq_steps(cbid, W, O.block_ldl(L64, 8), hat, Q)
    print(f"ldlq_panel_rvq {cbid} ({m}, {n}): {rep}")
    assert rep.steps == m * (n // 8) and rep.over == 0
    assert np.array_equal(hat, R.decode_f32(cbid, Q, R.DEFAULT_SCALE[cbid]).reshape(m, n))


@pytest.mark.parametrize("m,n", C.SHAPES)
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_tune_sweep(cbid, m, n):
    W, H, L64, hat0, _ = _fused(cbid, m, n, 0)
    _, _, _, hat1, Q1 = _fused(cbid, m, n, 1)
    rep = R.check_rvq_tune_steps(cbid, W, H, hat0, hat1, Q1)
    print(f"tune sweep {cbid} ({m}, {n}): {rep}")
    assert rep.steps == m * (n // 8) and rep.over == 0
    assert np.array_equal(hat1, R.decode_f32(cbid, Q1, R.DEFAULT_SCALE[cbid]).reshape(m, n))
    # the sweep may not raise the proxy loss by more than the stepwise route's sweep does on the same input
    Wt, Ht, Lt = (torch.from_numpy(a).to(DEV) for a in (W, H, L64.astype(np.float32)))
    s0, _ = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), _cb(cbid), 0)
    s1, _ = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), _cb(cbid), 1)
    rise_fused = C.proxy_loss(W, hat1, H) - C.proxy_loss(W, hat0, H)
    rise_step = C.proxy_loss(W, s1.cpu().numpy(), H) - C.proxy_loss(W, s0.cpu().numpy(), H)
    print(f"proxy loss change of one sweep: fused {rise_fused:.6e}, stepwise {rise_step:.6e}")
    assert max(rise_fused, 0.0) <= max(rise_step, 0.0)


def _oracle(cbid, iters):
    if (cbid, iters) not in _ORACLE:
        _ORACLE[(cbid, iters)] = O.ldlq(G["ldlq_E8P12_W"], G["ldlq_E8P12_H"], cbid, iters)
    return _ORACLE[(cbid, iters)]


@pytest.mark.parametrize("iters", [0, 1])
@pytest.mark.parametrize("route", ["panels", "stepwise"])
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_routes_agree_with_the_float64_oracle(cbid, route, iters, monkeypatch):
    """tests/test_gpu_quantize.py::test_ldlq_matches_reference's criteria against O.ldlq on the golden E8P12 (W, H) pair:
    the fused route called explicitly, and LDLQ with the switch off"""
    cb = _cb(cbid)
    W = torch.from_numpy(G["ldlq_E8P12_W"]).to(DEV)
    H = torch.from_numpy(G["ldlq_E8P12_H"]).to(DEV)
    L = torch.linalg.cholesky(H)
    if route == "stepwise":
        monkeypatch.setattr(quant, "_LDLQ_FUSED_RVQ", None)
        monkeypatch.delenv("QUIP_LDLQ_FUSED_RVQ", raising=False)
        assert quant.ldlq_route(W, cb) == "stepwise"
        run = quant.LDLQ
    else:
        run = quant.LDLQ_panels
    Wn, Hn = G["ldlq_E8P12_W"].astype(np.float64), G["ldlq_E8P12_H"].astype(np.float64)
    hat_ref, ref = _oracle(cbid, iters)
    e_ref = C.proxy_loss(Wn, hat_ref, Hn)
    for buf in (128, 16):
        hat, Q = run(W.clone(), H.clone(), L.clone(), cb, iters, buf_cols=buf)
        got = Q.cpu().numpy().astype(np.int64) & 0xffffffff
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


def _first_max_e81b(r, g):
    """arg max_c 2 r . g_c - |g_c|^2 in fp32 with the dot product summed left to right, every product and sum an fp32
    operation of its own (elementwise torch), the lowest index among equal scores"""
    dot = r[:, 0:1] * g[:, 0]
    for j in range(1, 8):
        dot = dot + r[:, j:j + 1] * g[:, j]
    score = 2.0 * dot - (g * g).sum(-1)
    best = score.max(dim=-1, keepdim=True).values
    ids = torch.arange(256, device=r.device).expand_as(score)
    return torch.where(score == best, ids, torch.full_like(ids, 256)).min(dim=-1).values


def _chain(cb, t, s):
    """the stepwise route's launches for targets t (N, 8), written out: e8p_quantize, the residual by a subtraction and a
    true division (the divisor a 0-dim device tensor, which torch does not turn into a reciprocal), the second search, and
    a + b * s by a multiplication and an addition.  -> (hat (N, 8), idx (N,) int64)"""
    sdev = torch.tensor(s, dtype=torch.float32, device=t.device)
    a, code_a = torch.ops.quip_lib.e8p_quantize(t.contiguous(), cb.grid_packed_abs)
    r = ((t - a) / sdev).contiguous()
    if cb.id == "E8P12RVQ4B":
        b, code_b = torch.ops.quip_lib.e8p_quantize(r, cb.grid_packed_abs)
        idx = (code_a << 16) | code_b
    else:
        g = cb.e81b_grid.to(torch.float32)
        code_b = _first_max_e81b(r, g)
        b = g[code_b]
        idx = (code_a << 8) | code_b
    return a + b * sdev, idx


def _check_same_as_chain(cbid, m, c, s, report=False):
    cb = _cb(cbid) if s is None else _cb(cbid, opt_resid_scale=s)
    s = cb.opt_resid_scale
    A, B, _, _ = _operands(m, c, False, seed=3)
    A[0] = 0.0
    B[0] = 0.0                                                          # ties at the origin: stage 1, and r = 0 for E81B
    hat, idx = _op(cb, A, B, torch.zeros(c, c, device=DEV), None)
    want_hat, want_idx = _chain(cb, (A + B).reshape(-1, 8), s)
    assert torch.equal(idx, want_idx.reshape(m, c // 8))
    assert torch.equal(hat, want_hat.reshape(m, c))
    if report:
        _, ix = cb.quantize((A + B).reshape(-1, 8))
        print(f"{cbid} ({m}, {c}): {(ix.reshape(m, c // 8) == idx).float().mean().item():.4f} of the indices equal "
              "cb.quantize's (which may divide by a Python scalar as a multiplication)")


@pytest.mark.parametrize("m,c", [(40, 128), (33, 48), (5, 8), (1, 16)])
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_same_two_searches_as_the_stepwise_chain(cbid, m, c):
    """M = 0 and no P: every group's target is A + B, and (hat, idx) are those of the written-out chain, bit for bit"""
    _check_same_as_chain(cbid, m, c, None, report=True)


@pytest.mark.parametrize("cbid", R.CBIDS)
def test_non_default_scale(cbid):
    """resid_scale = -1.0, which the reference's quantizer hands through when its own default is left alone"""
    _check_same_as_chain(cbid, 33, 48, -1.0)


def test_e81b_zero_residual_takes_entry_56():
    """r = 0: every score is -|g_c|^2, the only zero-norm entry wins; built here with a target that is a codeword"""
    cb = _cb("E8P12RVQ3B")
    g1 = torch.from_numpy(O.e8p_full_grid_f64()[[0, 513, 40000, 65535]].astype(np.float32)).to(DEV)
    A = g1.reshape(1, 32).contiguous()
    hat, idx = _op(cb, A, torch.zeros_like(A), torch.zeros(32, 32, device=DEV), None)
    assert (idx & 0xff).tolist() == [[56] * 4] and torch.equal(hat, A)
    assert float(np.abs(O.e81b_grid()[56]).max()) == 0.0


@pytest.mark.parametrize("c,with_p", [(128, False), (128, True), (48, False), (48, True), (8, False), (8, True)])
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_rows_are_independent_and_runs_repeat(cbid, c, with_p):
    cb = _cb(cbid)
    A, B, M, P = _operands(40, c, with_p)
    hat, idx = _op(cb, A, B, M, P)
    assert tuple(hat.shape) == (40, c) and tuple(idx.shape) == (40, c // 8) and idx.dtype == torch.int64
    hat2, idx2 = _op(cb, A, B, M, P)
    assert torch.equal(hat, hat2) and torch.equal(idx, idx2)
    parts = [_op(cb, A[r].contiguous(), B[r].contiguous(), M, P) for r in (slice(0, 7), slice(7, 40))]
    assert torch.equal(hat, torch.cat([p[0] for p in parts])) and torch.equal(idx, torch.cat([p[1] for p in parts]))
    assert torch.equal(hat.cpu(), torch.from_numpy(R.decode_f32(cbid, idx.cpu().numpy(), cb.opt_resid_scale)).reshape(40, c))


def test_operand_checks(monkeypatch):
    from quip_for_all_amd import capi
    cb = _cb("E8P12RVQ3B")
    g, e, s = cb.grid_packed_abs, cb.e81b_grid.to(torch.float32).contiguous(), cb.opt_resid_scale
    A, B, M, P = _operands(8, 16, True)
    op = torch.ops.quip_lib.ldlq_panel_rvq
    op(A, B, M, P, g, e, s)
    op(A, B, M, P, g, None, s)
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
    bad = [args + (grid2, s) for args in bad for grid2 in (e, None)]
    bad += [(A, B, M, P, g, e.half(), s), (A, B, M, P, g, e.double(), s),                                      # resid_grid
            (A, B, M, P, g, e[:128].contiguous(), s), (A, B, M, P, g, e.reshape(8, 256), s), (A, B, M, P, g, e.t(), s),
            (A, B, M, P, g, e.cpu(), s)]
    bad += [(A, B, M, P, g, grid2, v) for grid2 in (e, None)                                                   # resid_scale
            for v in (0.0, float("nan"), float("inf"), 1e-60, 1e60)]
    entered, check = [], capi.check
    monkeypatch.setattr(capi, "check", lambda rc, name: entered.append(name) or check(rc, name))
    for args in bad:
        with pytest.raises((ValueError, RuntimeError)):
            op(*args)
    assert entered == []                                     # every refusal came before the C entry, so before a launch
    op(A, B, M, P, g, e, s)
    assert entered == ["quip_ldlq_panel_rvq_f32"]
    torch.cuda.synchronize()


def _quant_layer(cbid, fin, fout, monkeypatch, switch):
    """QUIP.quant on one seeded nn.Linear with QUIP_LDLQ_FUSED_RVQ on or off -> (rel error, routes reported, layer, attr)"""
    from quip_for_all_amd.quip import QUIP
    monkeypatch.setattr(quant, "_LDLQ_FUSED_RVQ", None)
    monkeypatch.setenv("QUIP_LDLQ_FUSED_RVQ", "1" if switch else "0")
    routes, route_fn = [], quant.ldlq_route
    monkeypatch.setattr(quant, "ldlq_route", lambda Wr, cb: routes.append(route_fn(Wr, cb)) or routes[-1])
    torch.manual_seed(fin + fout)
    lin = torch.nn.Linear(fin, fout, bias=True).to(DEV)
    W0 = lin.weight.data.clone()
    q = QUIP(lin, _cb(cbid))
    q.add_batch(torch.randn(4, 64, fin, device=DEV))
    attr = q.quant(use_rand=True)
    rel = ((lin.weight.data - W0).norm() / W0.norm()).item()
    return rel, routes, lin, attr


@pytest.mark.parametrize("cbid,fin,fout", [("E8P12RVQ4B", 256, 256), ("E8P12RVQ4B", 256, 688), ("E8P12RVQ3B", 256, 256)])
def test_layer_quantiser_roundtrip_identity_on_the_fused_route(cbid, fin, fout, monkeypatch):
    """tests/test_gpu_quantize.py::test_layer_quantiser_roundtrip_identity with QUIP_LDLQ_FUSED_RVQ=1: QUIP.quant() took the
    fused route, hatW is a 4-bit-quality approximation of W (E8P12RVQ4B: relative error < 0.2, that test's bound), and
    nn.Linear(hatW)(x) == QuantLinear(x) up to fp16 rounding, so pack and decompress agree with hatWr.
    E8P12RVQ3B has no bound there; here it is the stepwise route's relative error on the same seeded layer plus 2 % of
    that value.  Measured on an MI355X at (256, 256): stepwise 0.256922, fused 0.256922 (bound
    0.262060); E8P12RVQ4B fused 0.146604 at (256, 256) and 0.149874 at (256, 688)."""
    import quip_for_all_amd as Q
    rel, routes, lin, attr = _quant_layer(cbid, fin, fout, monkeypatch, True)
    assert routes == ["panels"], routes
    if cbid == "E8P12RVQ4B":
        bound = 0.2
    else:
        rel_step, routes_step, _, _ = _quant_layer(cbid, fin, fout, monkeypatch, False)
        assert routes_step == ["stepwise"], routes_step
        bound = 1.02 * rel_step
    print(f"{cbid} ({fin}, {fout}) through QUIP.quant on the fused route: rel_error {rel:.6f}, bound {bound:.6f}")
    assert rel <= bound, (rel, bound)
    hatW = lin.weight.data.clone()
    ql = Q.QuantLinear(fin, fout, _cb(cbid), bias=True, use_rand=True).to(DEV)
    ql.pack(lin, attr)
    ql.wscale_float = ql.Wscale.mean().float().item()
    ql = ql.eval()
    x = torch.randn(7, fin, device=DEV).half()
    with torch.no_grad():
        y = ql(x).float()
        ref = torch.nn.functional.linear(x.float(), hatW.float(), lin.bias.float())
    tol = 4e-3 * ref.abs().max().item() + 2e-3
    assert (y - ref).abs().max().item() <= tol, ((y - ref).abs().max().item(), tol)
