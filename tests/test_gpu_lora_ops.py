"""The two LoRA launches on the device (csrc/lora_rows.hip.h) against their float64 statements (lora.shrink_ref /
expand_ref): every input mode, widths on both sides of the 512 elements a wave covers per sweep, ranks 8 .. 192, rows with
and without an adapter; rows that do not depend on their launch; a captured shrink + expand that follows its index tensor."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
N_ADAPTERS = 3
MODES = ["plain", "norm", "gate"]


def _indices(rows, seed):
    """-1 and the three adapters mixed; a single row takes an adapter"""
    if rows == 1:
        return torch.tensor([seed % N_ADAPTERS], dtype=torch.int32)
    g = torch.Generator().manual_seed(seed)
    idx = (torch.arange(rows) % (N_ADAPTERS + 1) - 1)[torch.randperm(rows, generator=g)]
    return idx.to(torch.int32)


def _shrink_inputs(rows, n_in, R, mode, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, n_in, generator=g).to(torch.float16)
    A = (torch.randn(N_ADAPTERS, R, n_in, generator=g) / n_in ** 0.5).to(torch.float16)
    kw = {}
    if mode == "norm":
        kw = {"rms_weight": (1.0 + 0.1 * torch.randn(n_in, generator=g)).to(torch.float16), "rms_eps": EPS}
    if mode == "gate":
        kw = {"gate": (3.0 * torch.randn(rows, n_in, generator=g)).clamp(-8.0, 8.0).to(torch.float16)}      # |g| <= 8
    return x, A, kw


def _dev(kw):
    return {k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in kw.items()}


def _check_shrink(rows, n_in, R, mode, seed):
    """|t - t64| <= 2^-24 (in + 16) sum |A_i xin_i| (any order of the in additions, the products and xin's own roundings)
    + 2^-19 |t64| for the norm factor (qk_norm_ref's rel) + sum |A_i xin_i| (|g_i| + 6) 2^-24 for the gate (__expf, the add,
    the 1-ulp reciprocal and the products)"""
    from quip_for_all_amd.lora import shrink_ref
    x, A, kw = _shrink_inputs(rows, n_in, R, mode, seed)
    idx = _indices(rows, seed)
    t = torch.ops.quip_lib.lora_shrink_rows(x.to(DEV), A.to(DEV), idx.to(DEV), **_dev(kw))
    assert t.dtype == torch.float32 and tuple(t.shape) == (rows, R)
    ref, mag, gmag = shrink_ref(x, A, idx, **kw)
    tol = 2.0 ** -24 * (n_in + 16) * mag + (2.0 ** -19 * np.abs(ref) if mode == "norm" else 0.0) + 2.0 ** -24 * gmag
    err = np.abs(t.cpu().numpy().astype(np.float64) - ref)
    assert np.all(err <= tol), (rows, n_in, R, mode, float((err - tol).max()))
    none = (idx < 0).numpy()
    assert not t.cpu().numpy()[none].any()                  # rows without an adapter: exactly zero
    return float(np.max(err / np.maximum(tol, 1e-300)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n_in", [8, 504, 512, 520, 688, 4104])
def test_shrink_against_float64(n_in, mode):
    """in: a single piece, a partial sweep, exactly one sweep, one piece over, TINY's ffn, several sweeps of the staging
    loop and one piece; every rank count and row count with each"""
    worst = 0.0
    for R in (8, 16, 64, 192):
        for rows in (1, 3, 31, 33):
            worst = max(worst, _check_shrink(rows, n_in, R, mode, seed=n_in + R + rows))
    print(f"lora_shrink_rows in = {n_in}, {mode}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("n_in,mode", [(12296, "norm"), (28672, "gate"), (28672, "norm")])
def test_shrink_with_more_than_48_kb_of_staged_row(n_in, mode):
    """the staged row takes the dynamic-LDS limit the launch layer has to raise (48 KB: 12288 elements), up to the widest
    input served (28672: 112 KB)"""
    _check_shrink(2, n_in, 8, mode, seed=n_in)


def _ulp16(v):
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


SEGMENTS = {1: [(None, 8)], 2: [(None, 16), (264, 8)], 3: [(None, 8), (0, 16), (248, 64)]}      # (out_j or the case's, R_j)


@pytest.mark.parametrize("nseg", [1, 2, 3])
@pytest.mark.parametrize("out", [8, 248, 256, 264])
def test_expand_against_float64(out, nseg):
    """out: one short tile, one thread short of a tile, a full tile, a tile and 8; 1 .. 3 segments of different widths and
    ranks, the middle one of three skipped (out_j = 0).  Bound: half an fp16 ulp of the result + 2^-24 (R + 3) (|y| + |scale|
    sum |B t|)"""
    from quip_for_all_amd.lora import expand_ref
    segs = [(out if o is None else o, R) for o, R in SEGMENTS[nseg]]
    Rt = sum(R for _, R in segs)
    r0 = [sum(R for _, R in segs[:j]) for j in range(nseg)]
    for rows in (1, 33):
        g = torch.Generator().manual_seed(out + nseg + rows)
        idx = _indices(rows, out + rows)
        t = torch.randn(rows, Rt, generator=g)
        scale = (0.25 + 2.0 * torch.rand(N_ADAPTERS, 3, generator=g)).to(torch.float32)
        ys = [torch.randn(rows, o, generator=g).to(torch.float16) for o, _ in segs]
        Bs = [(torch.randn(N_ADAPTERS, o, R, generator=g) / R ** 0.5).to(torch.float16) for o, R in segs]
        yd = [y.to(DEV) for y in ys]
        assert torch.ops.quip_lib.lora_expand_rows(t.to(DEV), yd, [B.to(DEV) for B in Bs], scale.to(DEV), idx.to(DEV), r0) is None
        for j, (o, R) in enumerate(segs):
            ref, mag = expand_ref(ys[j], Bs[j], t, scale, idx, j, r0[j])
            got = yd[j].cpu().numpy().astype(np.float64)
            tol = 0.5 * _ulp16(ref) + 2.0 ** -24 * (R + 3) * mag
            err = np.abs(got - ref)
            assert np.all(err <= tol), (out, nseg, rows, j, float((err - tol).max()))
            none = (idx < 0).numpy()
            assert torch.equal(yd[j].cpu()[none].view(torch.int16), ys[j][none].view(torch.int16))


def test_rows_without_an_adapter_keep_a_poisoned_y():
    """index -1: the shrink writes zeros, the expand writes nothing -- a y filled with 0xA5 bytes keeps them"""
    import quip_for_all_amd.lora  # noqa: F401
    rows, n_in, R, out = 5, 520, 16, 264
    x, A, _ = _shrink_inputs(rows, n_in, R, "plain", 1)
    idx = torch.tensor([-1, 0, -1, 2, -1], dtype=torch.int32, device=DEV)
    t = torch.ops.quip_lib.lora_shrink_rows(x.to(DEV), A.to(DEV), idx)
    assert not t[[0, 2, 4]].any() and t[[1, 3]].abs().sum() > 0
    y = torch.full((rows, out), 0xA5, dtype=torch.uint8, device=DEV).repeat(1, 2).view(torch.float16)
    assert tuple(y.shape) == (rows, out)
    B = torch.randn(N_ADAPTERS, out, R, device=DEV).to(torch.float16)
    scale = torch.ones(N_ADAPTERS, 3, device=DEV)
    torch.ops.quip_lib.lora_expand_rows(t, [y], [B], scale, idx, [0])
    poison = y.view(torch.uint8)
    assert bool((poison[[0, 2, 4]] == 0xA5).all())
    assert not bool((poison[[1, 3]] == 0xA5).all())
    # an index past the last adapter is no adapter either (never a read past the stacks)
    idx2 = torch.tensor([N_ADAPTERS, 0, 7, 2, -3], dtype=torch.int32, device=DEV)
    t2 = torch.ops.quip_lib.lora_shrink_rows(x.to(DEV), A.to(DEV), idx2)
    assert torch.equal(t2, t)


@pytest.mark.parametrize("mode", MODES)
def test_a_row_does_not_depend_on_its_launch(mode):
    """row i of a 33-row launch == the same row launched alone == the same row at another place among other rows, bit for
    bit, through shrink and expand"""
    import quip_for_all_amd.lora  # noqa: F401
    rows, n_in, R, out = 33, 688, 24, 264
    x, A, kw = _shrink_inputs(rows, n_in, R, mode, 5)
    x, A, kw = x.to(DEV), A.to(DEV), _dev(kw)
    idx = _indices(rows, 3).to(DEV)
    g = torch.Generator().manual_seed(9)
    y0 = torch.randn(rows, out, generator=g).to(torch.float16).to(DEV)
    B = torch.randn(N_ADAPTERS, out, 16, generator=g).to(torch.float16).to(DEV)
    scale = torch.tensor([[0.5] * 3, [2.0] * 3, [1.25] * 3], device=DEV)

    def run(sel):
        k = dict(kw)
        if "gate" in k:
            k["gate"] = k["gate"][sel].contiguous()
        t = torch.ops.quip_lib.lora_shrink_rows(x[sel].contiguous(), A, idx[sel].contiguous(), **k)
        y = y0[sel].clone()
        torch.ops.quip_lib.lora_expand_rows(t, [y], [B], scale, idx[sel].contiguous(), [8])
        return t, y
    t_all, y_all = run(torch.arange(rows, device=DEV))
    perm = torch.randperm(rows, generator=g).to(DEV)
    t_perm, y_perm = run(perm)
    assert torch.equal(t_perm, t_all[perm]) and torch.equal(y_perm.view(torch.int16), y_all[perm].view(torch.int16))
    for i in (0, 7, 32):
        t1, y1 = run(torch.tensor([i], device=DEV))
        assert torch.equal(t1[0], t_all[i]) and torch.equal(y1[0].view(torch.int16), y_all[i].view(torch.int16)), i


def test_captured_shrink_and_expand_follow_the_index_tensor():
    """a hipGraph of shrink + expand reads row_adapter in place: rewritten between replays, the replay gives the bits of an
    eager run with the new indices"""
    from quip_for_all_amd.decode import capture_graph
    rows, n_in, R, out = 4, 512, 16, 256
    x, A, kw = _shrink_inputs(rows, n_in, R, "norm", 2)
    x, A, kw = x.to(DEV), A.to(DEV), _dev(kw)
    g = torch.Generator().manual_seed(4)
    y0 = torch.randn(rows, out, generator=g).to(torch.float16).to(DEV)
    B = torch.randn(N_ADAPTERS, out, R, generator=g).to(torch.float16).to(DEV)
    scale = torch.tensor([[0.5] * 3, [2.0] * 3, [1.25] * 3], device=DEV)
    idx = torch.tensor([0, 1, -1, 2], dtype=torch.int32, device=DEV)

    def body(index):
        y = y0.clone()
        torch.ops.quip_lib.lora_expand_rows(torch.ops.quip_lib.lora_shrink_rows(x, A, index, **kw), [y], [B], scale, index, [0])
        return y
    graph, y_static = capture_graph(lambda: body(idx), lambda: body(idx))
    seen = []
    for new in ([0, 1, -1, 2], [2, 2, 0, -1], [-1, -1, -1, -1], [1, 0, 2, 1]):
        idx.copy_(torch.tensor(new, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        want = body(torch.tensor(new, dtype=torch.int32, device=DEV))
        assert torch.equal(y_static.view(torch.int16), want.view(torch.int16)), new
        seen.append(y_static.clone())
    assert torch.equal(seen[2], y0) and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[3])


def test_op_refusals():
    import quip_for_all_amd.lora  # noqa: F401
    shrink, expand = torch.ops.quip_lib.lora_shrink_rows, torch.ops.quip_lib.lora_expand_rows
    h = lambda *s: torch.zeros(*s, dtype=torch.float16, device=DEV)  # noqa: E731
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="in = 12"):
        shrink(h(2, 12), h(3, 8, 12), i32(2))
    with pytest.raises(ValueError, match="R = 12"):
        shrink(h(2, 16), h(3, 12, 16), i32(2))
    with pytest.raises(ValueError, match="row_adapter"):
        shrink(h(2, 16), h(3, 8, 16), i32(3))
    with pytest.raises(ValueError, match="row_adapter"):
        shrink(h(2, 16), h(3, 8, 16), torch.zeros(2, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="not both"):
        shrink(h(2, 16), h(3, 8, 16), i32(2), h(16), 1e-5, h(2, 16))
    with pytest.raises(ValueError, match="gate"):
        shrink(h(2, 16), h(3, 8, 16), i32(2), None, 1e-5, h(3, 16))
    t, sc = torch.zeros(2, 16, device=DEV), torch.zeros(3, 3, device=DEV)
    with pytest.raises(ValueError, match="out_0 = 12"):
        expand(t, [h(2, 12)], [h(3, 12, 8)], sc, i32(2), [0])
    with pytest.raises(ValueError, match="segment 0"):
        expand(t, [h(2, 8)], [h(3, 8, 16)], sc, i32(2), [8])
    with pytest.raises(ValueError, match="scale"):
        expand(t, [h(2, 8)], [h(3, 8, 16)], torch.zeros(3, 2, device=DEV), i32(2), [0])
    with pytest.raises(ValueError, match="Bs"):
        expand(t, [h(2, 8)], [h(3, 16, 16)], sc, i32(2), [0])
