"""Per-head RMSNorm of q / k on the device (csrc/qk_norm.hip.h, csrc/attn_query.hip.h): quip_lib::qk_norm_rows against
the float64 interval of qk_norm.qk_norm_ref, and the two decode launches that fuse the norm (rope_attn_decode_qknorm,
rope_attn_decode_batched_qknorm) against qk_norm_rows followed by the plain launch, bit for bit."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6


def norm_inputs(rows, heads, kv_heads, hd, seed=0):
    """(q, k, q_weight, k_weight) on the CPU: randn rows and, from 5 rows on, an all-zero row, a row of +-60000, a row of
    fp16 subnormals and a row with one huge element; weights with negative, zero and large entries.  The host test
    (test_qk_norm_host.py) checks HF's own norm against qk_norm_ref on exactly these."""
    g = torch.Generator().manual_seed(1000 * rows + 10 * heads + kv_heads + hd + seed)
    q = torch.randn(rows, heads * hd, generator=g).half()
    k = torch.randn(rows, kv_heads * hd, generator=g).half()
    for t in (q, k):
        n = t.shape[1]
        sign = (torch.randint(0, 2, (n,), generator=g) * 2 - 1).half()
        kinds = [torch.zeros(n).half(), 60000.0 * sign,
                 (torch.randint(1, 1024, (n,), generator=g).float() * 2.0 ** -24).half() * sign,
                 torch.cat([torch.tensor([30000.0]), 0.01 * torch.randn(n - 1, generator=g)]).half()]
        for j, row in enumerate(kinds):      # from the last row backwards; row 0 stays randn (a one-row call: randn only)
            if rows - 1 - j >= 1:
                t[rows - 1 - j] = row
    qw = (1.0 + 0.5 * torch.randn(hd, generator=g)).half()
    kw = (1.0 + 0.5 * torch.randn(hd, generator=g)).half()
    qw[1], qw[2], qw[3], qw[5] = -1.5, 0.0, 900.0, -0.001
    kw[0], kw[7], kw[hd - 1] = 0.0, -300.0, 40000.0
    return q, k, qw, kw


SHAPES = [(4, 2, 128), (4, 4, 64), (8, 2, 64)]
ROWS = [1, 5, 70]


def _inside(y, x, w, hd):
    from quip_for_all_amd.qk_norm import qk_norm_ref
    lo, hi = qk_norm_ref(x.reshape(x.shape[0], -1, hd), w, EPS)
    y = y.cpu().reshape(lo.shape)
    assert not torch.isnan(y).any()
    bad = ~((y >= lo) & (y <= hi))
    assert not bad.any(), (int(bad.sum()), y[bad][:4], lo[bad][:4], hi[bad][:4])


@pytest.mark.parametrize("heads,kv_heads,hd", SHAPES)
@pytest.mark.parametrize("rows", ROWS)
def test_qk_norm_rows_inside_the_float64_interval(heads, kv_heads, hd, rows):
    import quip_for_all_amd.qk_norm  # noqa: F401
    q, k, qw, kw = norm_inputs(rows, heads, kv_heads, hd)
    # guard bytes around q and k, and a v that nobody may touch
    guard = 64
    buf = torch.full((guard + q.numel() + guard + k.numel() + guard,), 1234.0, dtype=torch.float16, device=DEV)
    qd = buf[guard:guard + q.numel()].view_as(q)
    kd = buf[2 * guard + q.numel():2 * guard + q.numel() + k.numel()].view_as(k)
    qd.copy_(q)
    kd.copy_(k)
    v = torch.randn(rows, kv_heads * hd, device=DEV).half()
    v0 = v.clone()
    assert torch.ops.quip_lib.qk_norm_rows(qd, kd, qw.to(DEV), kw.to(DEV), hd, EPS) is None
    torch.cuda.synchronize()
    _inside(qd, q, qw, hd)
    _inside(kd, k, kw, hd)
    if rows >= 5:
        assert torch.equal(qd[rows - 1], torch.zeros_like(qd[0]))       # the all-zero row: 0, not NaN
    g = buf.cpu()
    for a, b in ((0, guard), (guard + q.numel(), 2 * guard + q.numel()), (g.numel() - guard, g.numel())):
        assert torch.equal(g[a:b], torch.full((guard,), 1234.0, dtype=torch.float16))
    assert torch.equal(v, v0)


@pytest.mark.parametrize("heads,kv_heads,hd", SHAPES)
def test_qk_norm_rows_heads_do_not_see_their_neighbours(heads, kv_heads, hd):
    """change one head (HD 64: it shares a 16-lane row with its neighbour) and every other head keeps its bits"""
    import quip_for_all_amd.qk_norm  # noqa: F401
    q, k, qw, kw = norm_inputs(5, heads, kv_heads, hd, seed=1)
    qw, kw = qw.to(DEV), kw.to(DEV)
    q0, k0 = q.to(DEV), k.to(DEV)
    torch.ops.quip_lib.qk_norm_rows(q0, k0, qw, kw, hd, EPS)
    for t, row, head in (("q", 0, 1), ("q", 2, 0), ("k", 0, kv_heads - 1), ("k", 3, 0)):
        q1, k1 = q.clone(), k.clone()
        (q1 if t == "q" else k1)[row, head * hd:(head + 1) * hd] = 1000.0
        q1, k1 = q1.to(DEV), k1.to(DEV)
        torch.ops.quip_lib.qk_norm_rows(q1, k1, qw, kw, hd, EPS)
        same_q, same_k = q1 == q0, k1 == k0
        (same_q if t == "q" else same_k)[row, head * hd:(head + 1) * hd] = True
        assert same_q.all() and same_k.all(), (t, row, head)
        assert not torch.equal((q1 if t == "q" else k1)[row, head * hd:(head + 1) * hd],
                               (q0 if t == "q" else k0)[row, head * hd:(head + 1) * hd])


def test_qk_norm_rows_refusals():
    import quip_for_all_amd.qk_norm  # noqa: F401
    op = torch.ops.quip_lib.qk_norm_rows
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device=DEV)  # noqa: E731
    w = h(64)
    op(h(2, 256), h(2, 128), w, w, 64, EPS)                                       # (the accepted call)
    with pytest.raises(ValueError):
        op(h(2, 512)[:, ::2], h(2, 128), w, w, 64, EPS)                           # non-contiguous q
    with pytest.raises(ValueError):
        op(h(2, 256), h(2, 256)[:, :128], w, w, 64, EPS)                          # non-contiguous k
    with pytest.raises(ValueError):
        op(h(2, 256).float(), h(2, 128), w, w, 64, EPS)                           # dtype
    with pytest.raises(ValueError):
        op(h(2, 256), h(2, 128), w.float(), w, 64, EPS)
    with pytest.raises(ValueError):
        op(h(2, 96 * 2), h(2, 96), h(96), h(96), 96, EPS)                         # head_dim outside {64, 128}
    with pytest.raises(ValueError):
        op(h(2, 256), h(2, 128), h(32), h(32), 32, EPS)
    with pytest.raises(ValueError):
        op(h(2, 256 + 8), h(2, 128), w, w, 64, EPS)                               # width not a multiple of head_dim
    with pytest.raises(ValueError):
        op(h(2, 256), h(2, 96), w, w, 64, EPS)
    with pytest.raises(ValueError):
        op(h(2, 256), h(3, 128), w, w, 64, EPS)                                   # rows differ
    with pytest.raises(ValueError):
        op(h(2, 256), h(2, 128), h(128), w, 64, EPS)                              # weight length


def _tables(max_len, hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


def _weights(hd, g):
    return ((1.0 + 0.3 * torch.randn(hd, generator=g)).half().to(DEV), (1.0 + 0.3 * torch.randn(hd, generator=g)).half().to(DEV))


@pytest.mark.parametrize("window", [0, 16])
@pytest.mark.parametrize("heads,kv_heads,hd", [(4, 4, 64), (8, 2, 64), (4, 4, 128), (8, 2, 128)])
def test_fused_decode_equals_norm_rows_then_plain_launch(heads, kv_heads, hd, window):
    """bs = 1, every position class (0, 1, inside one workgroup, around the split threshold), with the workspace (256 and
    300 run in split mode): out and both caches, bit for bit"""
    import quip_for_all_amd.qk_norm  # noqa: F401
    from quip_for_all_amd.register_lib import rope_attn_workspace
    max_len = 320
    g = torch.Generator().manual_seed(heads * 7 + hd + window)
    cos, sin = _tables(max_len, hd)
    qw, kw = _weights(hd, g)
    ws = rope_attn_workspace(heads, hd, DEV)
    kc0 = torch.randn(kv_heads, max_len, hd, generator=g).half().to(DEV)
    vc0 = torch.randn(kv_heads, max_len, hd, generator=g).half().to(DEV)
    for pos in (0, 1, 37, 255, 256, 300):
        q = (2.0 * torch.randn(heads, hd, generator=g)).half().to(DEV)
        k = (2.0 * torch.randn(kv_heads, hd, generator=g)).half().to(DEV)
        v = torch.randn(kv_heads, hd, generator=g).half().to(DEV)
        p = torch.tensor([pos], device=DEV)
        for w in (ws, None):
            kc1, vc1, kc2, vc2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
            q0, k0 = q.clone(), k.clone()
            fused = torch.ops.quip_lib.rope_attn_decode_qknorm(q, k, v, cos, sin, p, kc1, vc1, w, window, qw, kw, EPS)
            assert torch.equal(q, q0) and torch.equal(k, k0)                    # (the fused launch leaves q and k alone)
            qn, kn = q.reshape(1, -1).clone(), k.reshape(1, -1).clone()
            torch.ops.quip_lib.qk_norm_rows(qn, kn, qw, kw, hd, EPS)
            plain = torch.ops.quip_lib.rope_attn_decode(qn.view(heads, hd), kn.view(kv_heads, hd), v, cos, sin, p, kc2, vc2, w,
                                                        window)
            assert torch.equal(fused, plain), (pos, w is None)
            assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2), (pos, w is None)
            assert not torch.equal(kc1[:, pos], kc0[:, pos])


@pytest.mark.parametrize("heads,kv_heads,hd", [(4, 2, 64), (4, 2, 128)])
def test_fused_batched_decode_equals_norm_rows_then_plain_launch(heads, kv_heads, hd):
    """B = 3 at positions (0, 41, 299), with the workspace (299: split mode); then slot 1 at pos = max_len: NaN heads, no
    write, the other slots unchanged"""
    import quip_for_all_amd.qk_norm  # noqa: F401
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    B, max_len = 3, 304
    g = torch.Generator().manual_seed(heads + hd)
    cos, sin = _tables(max_len, hd)
    qw, kw = _weights(hd, g)
    ws = rope_attn_batched_workspace(B, heads, hd, DEV)
    kc0 = torch.randn(B, kv_heads, max_len, hd, generator=g).half().to(DEV)
    vc0 = torch.randn(B, kv_heads, max_len, hd, generator=g).half().to(DEV)
    q = (2.0 * torch.randn(B, heads, hd, generator=g)).half().to(DEV)
    k = (2.0 * torch.randn(B, kv_heads, hd, generator=g)).half().to(DEV)
    v = torch.randn(B, kv_heads, hd, generator=g).half().to(DEV)

    def both(pos):
        p = torch.tensor(pos, device=DEV)
        kc1, vc1, kc2, vc2 = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
        fused = torch.ops.quip_lib.rope_attn_decode_batched_qknorm(q, k, v, cos, sin, p, kc1, vc1, ws, 0, qw, kw, EPS)
        qn, kn = q.reshape(B, -1).clone(), k.reshape(B, -1).clone()
        torch.ops.quip_lib.qk_norm_rows(qn, kn, qw, kw, hd, EPS)
        plain = torch.ops.quip_lib.rope_attn_decode_batched(qn.view(B, heads, hd), kn.view(B, kv_heads, hd), v, cos, sin, p,
                                                            kc2, vc2, ws, 0)
        assert torch.equal(fused.view(torch.int16), plain.view(torch.int16))    # (bits: NaN rows included)
        assert torch.equal(kc1, kc2) and torch.equal(vc1, vc2)
        return fused, kc1, vc1
    good, kcg, vcg = both([0, 41, 299])
    assert not torch.isnan(good).any()
    # every slot: the bits of the bs = 1 fused launch on that slot alone
    from quip_for_all_amd.register_lib import rope_attn_workspace
    ws1 = rope_attn_workspace(heads, hd, DEV)
    for b, pos in enumerate([0, 41, 299]):
        kc1, vc1 = kc0[b].clone(), vc0[b].clone()
        one = torch.ops.quip_lib.rope_attn_decode_qknorm(q[b], k[b], v[b], cos, sin, torch.tensor([pos], device=DEV), kc1, vc1,
                                                         ws1, 0, qw, kw, EPS)
        assert torch.equal(one, good[b]) and torch.equal(kc1, kcg[b]) and torch.equal(vc1, vcg[b])
    out, kc, vc = both([0, max_len, 299])
    assert torch.isnan(out[1]).all()
    assert torch.equal(kc[1], kc0[1]) and torch.equal(vc[1], vc0[1])
    assert torch.equal(out[0], good[0]) and torch.equal(out[2], good[2])
    assert torch.equal(kc[0], kcg[0]) and torch.equal(kc[2], kcg[2])


@pytest.mark.parametrize("heads,kv_heads,hd,pos", [(8, 2, 128, 200), (4, 4, 64, 130)])
def test_fused_decode_matches_float64(heads, kv_heads, hd, pos):
    """norm, rotation and softmax attention as one float64 expression; the tolerance of test_rope_attn_decode_matches_torch"""
    import quip_for_all_amd.qk_norm  # noqa: F401
    g = torch.Generator().manual_seed(pos + heads)
    max_len = pos + 9
    cos, sin = _tables(max_len, hd)
    qw, kw = _weights(hd, g)
    q = torch.randn(heads, hd, generator=g).half().to(DEV)
    k = torch.randn(kv_heads, hd, generator=g).half().to(DEV)
    v = torch.randn(kv_heads, hd, generator=g).half().to(DEV)
    kc = torch.randn(kv_heads, max_len, hd, generator=g).half().to(DEV)
    vc = torch.randn(kv_heads, max_len, hd, generator=g).half().to(DEV)
    kc2, vc2 = kc.clone(), vc.clone()
    out = torch.ops.quip_lib.rope_attn_decode_qknorm(q, k, v, cos, sin, torch.tensor([pos], device=DEV), kc2, vc2, None, 0,
                                                     qw, kw, EPS)

    def norm(x, w):
        x = x.double()
        return x / torch.sqrt((x * x).mean(-1, keepdim=True) + EPS) * w.double()

    def rope(x):
        d = hd // 2
        rot = torch.cat([-x[..., d:], x[..., :d]], -1)
        return x * cos[pos].double() + rot * sin[pos].double()
    qr, kr = rope(norm(q, qw)), rope(norm(k, kw))
    assert (kc2[:, pos].double() - kr).abs().max().item() <= 2.0 ** -10 * max(1.0, kr.abs().max().item())   # (three fp16 roundings)
    assert torch.equal(vc2[:, pos], v)
    K, V = kc.double(), vc.double()
    K[:, pos], V[:, pos] = kr, v.double()
    rep = heads // kv_heads
    K = K[:, :pos + 1].repeat_interleave(rep, 0)
    V = V[:, :pos + 1].repeat_interleave(rep, 0)
    s = torch.einsum("hd,htd->ht", qr, K) / math.sqrt(hd)
    ref = torch.einsum("ht,htd->hd", torch.softmax(s, -1), V)
    err = (out.double() - ref).abs().max().item()
    print(f"fused qk-norm decode vs float64 (hd {hd}, pos {pos}): max abs err {err:.3e}")
    assert err <= 2e-3 * max(1.0, ref.abs().max().item()), err
