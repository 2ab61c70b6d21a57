"""The routed MLP half of a sparse-MoE block (quip_for_all_amd/moe.py; csrc/e8p_skinny_moe.hip, moe_rows.hip.h): router and
sort against float64, the routed product against the single skinny launch and float64, QuantMoeMlp.forward_rows against a
float64 Mixtral MLP, and a captured decoder step replayed on tokens that select other experts."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HIDDEN, FFN, EPS = 256, 512, 1e-5


@pytest.fixture(scope="module")
def Q():
    import __graft_entry__ as g
    g.build()
    import quip_for_all_amd as Q
    from quip_for_all_amd import moe  # noqa: F401  (defines the ops)
    return Q


def _f16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float16)).to(DEV)


def _router_ref(h, ln, wg, top_k, renorm=True):
    """float64: xn, logits, renormalised top-k weights, ids (lower index on a tie), the host sort, the bound's delta"""
    h, ln, wg = (np.asarray(a, np.float64) for a in (h, ln, wg))
    xn = h / np.sqrt((h * h).mean(-1, keepdims=True) + EPS) * ln
    logits = xn @ wg.T
    order = np.argsort(-logits, axis=-1, kind="stable")
    ids = order[:, :top_k]
    p = np.exp(logits - logits.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    w = np.take_along_axis(p, ids, -1)
    if renorm:
        w = w / w.sum(-1, keepdims=True)
    pairs = sorted((int(e), r, j) for r in range(h.shape[0]) for j, e in enumerate(ids[r]))
    E = wg.shape[0]
    start = np.searchsorted([e for e, _, _ in pairs], np.arange(E + 1)).astype(np.int32)
    pair_of = np.array([r * top_k + j for _, r, j in pairs], np.int32)
    delta = 2.0 ** -11 * np.abs(logits).max(-1) + h.shape[1] * 2.0 ** -24 * (np.abs(xn) @ np.abs(wg).T).max(-1)
    return xn, logits, ids, w, start, pair_of, delta


def _margin_ok(logits, top_k):
    """every row's k-th and (k + 1)-th logits differ by more than 8 fp16 ulps of the larger"""
    s = -np.sort(-logits, axis=-1)
    if top_k == logits.shape[1]:
        return np.ones(len(s), bool)
    big = np.maximum(np.abs(s[:, top_k - 1]), np.abs(s[:, top_k]))
    return s[:, top_k - 1] - s[:, top_k] > 8 * 2.0 ** (np.floor(np.log2(big)) - 10)


def _router_inputs(M, E, top_k, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    h = rng.standard_normal((M, HIDDEN)).astype(np.float16)
    ln = (1 + 0.05 * rng.standard_normal(HIDDEN)).astype(np.float16)
    wg = (rng.standard_normal((E, HIDDEN)) / 4).astype(np.float16)
    for _ in range(20):      # rows too close to a tie are drawn again; the margin is asserted below
        bad = ~_margin_ok(_router_ref(h, ln, wg, top_k)[1], top_k)
        h[bad] = rng.standard_normal((int(bad.sum()), HIDDEN)).astype(np.float16)
    return h, ln, wg, rng


@pytest.mark.parametrize("M,E,top_k", [(1, 8, 2), (2, 3, 1), (17, 8, 2), (31, 3, 2), (31, 8, 1)])
def test_router_and_sort_against_float64(Q, M, E, top_k):
    h, ln, wg, rng = _router_inputs(M, E, top_k, 100 + M + E)
    su = [rng.choice([-1.0, 1.0], (E, HIDDEN)).astype(np.float16), None]
    xn, logits, ids, w, start, pair_of, delta = _router_ref(h, ln, wg, top_k)
    assert _margin_ok(logits, top_k).all(), "test construction: a row within 8 fp16 ulps of a tie"
    xs, st, po, wt = torch.ops.quip_lib.moe_route_rows(_f16(h), _f16(ln), _f16(wg), _f16(su[0]), None, top_k, 2, True, EPS)
    st, po, wt = st.cpu().numpy(), po.cpu().numpy(), wt.cpu().numpy().astype(np.float64)
    assert np.array_equal(st, start) and np.array_equal(po, pair_of), (st, start, po, pair_of)
    err = np.abs(wt - w.reshape(-1)[pair_of])
    print(f"M {M} E {E} top_k {top_k}: max |w - w_ref| / 2 delta = {(err / (2 * delta[pair_of // top_k])).max():.3f}")
    assert (err <= 2 * delta[pair_of // top_k]).all()
    e_of = np.repeat(np.arange(E), np.diff(start))
    for g in range(2):       # the signed rows: one fp16 rounding of xn (and the norm factor's fp32)
        want = xn[pair_of // top_k] * (1.0 if su[g] is None else su[g].astype(np.float64)[e_of])
        assert (np.abs(xs[g].float().cpu().numpy() - want) <= 2.0 ** -10 * np.abs(want) + 1e-6).all()


def test_router_tie_takes_the_lower_index(Q):
    h = np.ones((2, HIDDEN), np.float16)
    wg = np.zeros((4, HIDDEN), np.float16)
    wg[1, :8] = wg[3, :8] = 0.25
    wg[2, :8] = 0.125
    _, st, po, wt = torch.ops.quip_lib.moe_route_rows(_f16(h), _f16(np.ones(HIDDEN)), _f16(wg), None, None, 2, 1, True, EPS)
    assert st.tolist() == [0, 0, 2, 2, 4] and po.tolist() == [0, 2, 1, 3] and wt.tolist() == [0.5] * 4
    _, st, po, _ = torch.ops.quip_lib.moe_route_rows(_f16(h), _f16(np.ones(HIDDEN)), _f16(wg), None, None, 1, 1, True, EPS)
    assert st.tolist() == [0, 0, 2, 2, 2] and po.tolist() == [0, 1]


def test_nan_and_inf_rows_stay_with_their_own_pairs(Q):
    """rows 1 (NaN) and 3 (inf): in-range ids and NaN outputs for their own pairs, every other row keeps its bits"""
    mlp, ln = _mlp(Q, 8, 2, 21)
    h = torch.randn(5, HIDDEN, generator=torch.Generator().manual_seed(9)).to(torch.float16).to(DEV)
    bad = h.clone()
    bad[1, 7], bad[3, 0] = float("nan"), float("inf")
    with torch.no_grad():
        clean, out = mlp.forward_rows(h, ln, EPS), mlp.forward_rows(bad, ln, EPS)
        _, start, pair_of, _ = torch.ops.quip_lib.moe_route_rows(bad, ln, mlp.router, None, None, 2, 1, True, EPS)
    assert sorted(pair_of.tolist()) == list(range(10)) and start[0] == 0 and start[-1] == 10 and (start[1:] >= start[:-1]).all()
    assert torch.isnan(out[[1, 3]]).all() and torch.equal(out[[0, 2, 4]], clean[[0, 2, 4]])


# rows per expert: empty experts, all pairs on one expert, M_e = 1 at both ends of the sorted order
@pytest.mark.parametrize("M,counts", [(1, [0, 1, 0, 0, 1, 0, 0, 0]), (17, [0, 17, 0]), (17, [17, 0, 17]),
                                      (31, [1, 0, 29, 31, 0, 0, 0, 1]), (2, [1, 2, 1]), (16, [16, 0, 5, 11])])
@pytest.mark.parametrize("n,k", [(512, 256), (258, 512)])
def test_routed_product_against_the_single_launch_and_float64(Q, M, counts, n, k):
    from oracle import quip_oracle as O
    from tests.test_gpu_ops import _mm_tol
    E, P, G = len(counts), sum(counts), 2
    rng = np.random.Generator(np.random.PCG64(7 + M + n))
    q = [torch.from_numpy(rng.integers(-32768, 32768, (E, n, k // 8)).astype(np.int16)).to(DEV) for _ in range(G)]
    x = _f16(rng.standard_normal((G, P, k)))
    scale = torch.from_numpy(rng.uniform(0.01, 0.1, (G, E)).astype(np.float32)).to(DEV)
    start = torch.tensor(np.concatenate([[0], np.cumsum(counts)]), dtype=torch.int32, device=DEV)
    grid = Q.codebook.codebook_id["E8P12"](inference=True).to(DEV).grid_packed_abs
    y = torch.full((G, P, n), float("nan"), dtype=torch.float16, device=DEV)
    y.copy_(torch.ops.quip_lib.mm_skinny_moe(x, q, scale, start, M, 0, grid))
    worst = 0.0
    for g in range(G):
        for e in range(E):
            s0, s1 = int(start[e]), int(start[e + 1])
            if s1 == s0:
                continue
            one = torch.ops.quip_lib.e8p_mm_skinny(x[g, s0:s1].contiguous(), q[g][e].contiguous(), grid)
            assert torch.equal(y[g, s0:s1], (one.float() * scale[g, e]).to(torch.float16)), (g, e)
            W = O.decompress_e8p(q[g][e].cpu().numpy()).astype(np.float64)
            x64 = x[g, s0:s1].cpu().numpy().astype(np.float64)
            y64 = x64 @ W.T
            sc = float(scale[g, e])
            err = np.abs(y[g, s0:s1].float().cpu().numpy() - sc * y64)
            # (the bound of mm_skinny, scaled, and the second fp16 rounding behind the scale)
            tol = sc * _mm_tol(x64, W, y64) + 2.0 ** -11 * np.abs(sc * y64) + 1e-7
            worst = max(worst, float((err / tol).max()))
    print(f"M {M} counts {counts} n {n} k {k}: worst error / tolerance {worst:.3f}")
    assert worst <= 1.0


def _mlp(Q, E, top_k, seed):
    from quip_for_all_amd import decode as D
    from quip_for_all_amd.moe import QuantMoeMlp
    g = torch.Generator().manual_seed(seed)
    experts = [(D.random_quant_linear(HIDDEN, FFN, generator=g, device=DEV), D.random_quant_linear(HIDDEN, FFN, generator=g, device=DEV),
                D.random_quant_linear(FFN, HIDDEN, generator=g, device=DEV)) for _ in range(E)]
    router = (torch.randn(E, HIDDEN, generator=g) / 4).to(torch.float16)
    ln = (1 + 0.05 * torch.randn(HIDDEN, generator=g)).to(torch.float16).to(DEV)
    return QuantMoeMlp(router, experts, top_k).to(DEV).eval(), ln


def _mlp_ref(mlp, ln, h):
    """HF Mixtral's block in float64 on the modules' dense weights (calc_weight): h + sum_k w_k w2(silu(w1 xn) * w3 xn)"""
    def lin(m, x):
        W = m.calc_weight(cache=False).double().cpu().numpy()
        y = ((x * m.SU.detach().double().cpu().numpy()) @ W)[:, :m.out_features]
        return y * m.SV.detach().double().cpu().numpy()
    h64 = h.double().cpu().numpy()
    xn, logits, ids, w, *_ = _router_ref(h64, ln.double().cpu().numpy(), mlp.router.double().cpu().numpy(), mlp.top_k)
    assert _margin_ok(logits, mlp.top_k).all(), "test construction: a row within 8 fp16 ulps of a tie"
    out = h64.copy()
    for r in range(h64.shape[0]):
        for j, e in enumerate(ids[r]):
            w1, w3, w2 = mlp.experts[int(e)]
            a = lin(w1, xn[r:r + 1])
            out[r] += w[r, j] * lin(w2, a / (1 + np.exp(-a)) * lin(w3, xn[r:r + 1]))[0]
    return out


# Two module stages in sequence (gate / up, then down), each within the 4 fp16 ulps of its output's scale the decoder
# tests budget per module (tests/test_gpu_decode.py: deep_bound_ulps), independent, so in quadrature; + 2 for the roundings
# this path adds (the signed rows, the product rounded in front of its scale) and the fp16 store: 4 sqrt(2) + 2
MLP_ULPS = 4.0 * math.sqrt(2.0) + 2.0


# (M = 32: beyond the routed launches, the loop over the experts on the modules' own forward)
@pytest.mark.parametrize("M,E,top_k", [(1, 8, 2), (2, 3, 1), (17, 8, 2), (31, 3, 2), (32, 3, 2)])
def test_mlp_half_against_float64_model(Q, M, E, top_k):
    from tests.test_gpu_decode import _ulps_of_rms
    mlp, ln = _mlp(Q, E, top_k, 3 + E)
    gen = torch.Generator().manual_seed(50 + M)
    h = torch.randn(M, HIDDEN, generator=gen).to(torch.float16)
    for _ in range(20):      # rows too close to a tie are drawn again; _mlp_ref asserts the margin
        bad = ~_margin_ok(_router_ref(h.numpy(), ln.cpu().numpy(), mlp.router.cpu().numpy(), top_k)[1], top_k)
        h[torch.from_numpy(bad)] = torch.randn(int(bad.sum()), HIDDEN, generator=gen).to(torch.float16)
    h = h.to(DEV)
    with torch.no_grad():
        got = mlp.forward_rows(h, ln, EPS).double().cpu().numpy()
        ref = _mlp_ref(mlp, ln, h)
    u = _ulps_of_rms(got, ref)
    print(f"moe mlp M {M} E {E} top_k {top_k}: max {u:.2f} fp16 ulps of rms(out) (bound {MLP_ULPS:.2f})")
    assert u <= MLP_ULPS, u
    for (w1, _, _), i in zip(mlp.experts, range(E)):      # the modules' codes are views of the stack
        assert w1.Qidxs.data_ptr() == mlp.q_w1[i].data_ptr()


def test_captured_decoder_step_serves_other_experts(Q):
    """one step of a tiny MoE decoder captured in a graph, replayed on tokens that select different experts: logits, the next
    token and the cache rows are those of the eager step each time; the engines are off on such a model"""
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=HIDDEN, ffn=FFN, layers=2, heads=4, kv_heads=2, vocab=512, n_experts=8, top_k=2)
    dec = D.LlamaDecoder(shape, max_len=16, device=DEV, seed=4)
    assert dec.moe and not (dec.block_eng or dec.ffn_eng or dec.chain or dec.fused_prologue or dec.attn_z or dec._token_tail_on())
    with pytest.raises(NotImplementedError, match="enable_lora"):
        dec.enable_lora()
    toks, routes = [5, 77, 300, 411], set()
    with torch.no_grad():
        eager = []
        for t in toks:      # every token at position 3 of the same three-token prefix
            dec.reset(1)
            for _ in range(3):
                dec.step()
            dec.tok.fill_(t)
            x = dec.embed[dec.tok]
            routes.add(tuple(torch.ops.quip_lib.moe_route_rows(x, dec.layers[0]["ln2"], dec.layers[0]["moe"].router, None, None,
                                                                2, 1, True, shape.rms_eps)[1].tolist()))
            logits = dec.step().clone()
            eager.append((logits, dec.kcache[:, :, 3].clone(), dec.vcache[:, :, 3].clone()))
        assert len(routes) > 1, "test construction: every token selects the same experts"
        dec.capture()
        for _ in range(2):
            for t, (logits, krow, vrow) in zip(toks, eager):
                dec.reset(1)
                for _ in range(3):
                    dec.graph.replay()
                dec.tok.fill_(t)
                dec.graph.replay()
                assert torch.equal(dec.step_logits, logits)
                assert torch.equal(dec.kcache[:, :, 3], krow) and torch.equal(dec.vcache[:, :, 3], vrow)
