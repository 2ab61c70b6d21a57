"""Batched decode on the GPU: the batched attention launch against B single-sequence launches (bit for bit), the greedy
tail over B rows against torch.argmax, and BatchDecoder against the bs=1 decoder -- exactly where every product takes
the exact rows-mode path, within the model-level bound where the skinny fp16 kernel serves the rows."""
import numpy as np
import pytest
import torch

from tests.test_gpu_decode import _ulps_of_rms, deep_bound_ulps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 320
# ragged positions: both sides of the split threshold (256), the first and the last cache row
POSITIONS = {1: [300], 3: [0, 256, MAX_LEN - 1],
             16: [0, 255, 256, 300, MAX_LEN - 1, 1, 7, 63, 64, 200, 257, 270, 288, 310, 318, 100]}


def _tables(max_len, hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


def _inputs(B, heads, kvh, hd, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).half().to(DEV)  # noqa: E731
    return r(B, heads, hd), r(B, kvh, hd), r(B, kvh, hd), r(B, kvh, MAX_LEN, hd), r(B, kvh, MAX_LEN, hd)


@pytest.mark.parametrize("heads,kvh,hd", [(32, 32, 128), (8, 2, 128), (4, 4, 64), (64, 8, 128)])
def test_batched_attention_equals_single_sequence_launches(heads, kvh, hd):
    """output and both caches of every sequence == quip_rope_attn_decode_window_f16 on that sequence alone, with and
    without workspace (split mode from 256 positions) and with a window; three launches back to back on one workspace
    (the arrival counters return to zero)"""
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    from quip_for_all_amd.register_lib import rope_attn_workspace
    cos, sin = _tables(MAX_LEN, hd)
    ws1 = rope_attn_workspace(heads, hd, DEV)
    for B, plist in POSITIONS.items():
        q, k, v, kc, vc = _inputs(B, heads, kvh, hd, seed=B + heads)
        pos = torch.tensor(plist, device=DEV)
        wsb = rope_attn_batched_workspace(B, heads, hd, DEV)
        for window in (0, 40):
            for use_ws in (False, True):
                ref = []
                for b in range(B):
                    kc1, vc1 = kc[b].clone(), vc[b].clone()
                    o1 = torch.ops.quip_lib.rope_attn_decode(q[b], k[b], v[b], cos, sin, pos[b:b + 1], kc1, vc1,
                                                             ws1 if use_ws else None, window)
                    ref.append((o1, kc1, vc1))
                for _ in range(3 if use_ws else 1):
                    kcb, vcb = kc.clone(), vc.clone()
                    out = torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, cos, sin, pos, kcb, vcb,
                                                                      wsb if use_ws else None, window)
                    for b, (o1, kc1, vc1) in enumerate(ref):
                        what = (B, b, plist[b], window, use_ws)
                        assert torch.equal(out[b], o1), what
                        assert torch.equal(kcb[b], kc1) and torch.equal(vcb[b], vc1), what
        assert int(wsb[-B * heads * 4:].view(torch.int32).abs().sum()) == 0      # counters back at zero


@pytest.mark.parametrize("bad", [MAX_LEN, -1])
def test_out_of_range_position_affects_only_its_own_sequence(bad):
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    heads, kvh, hd, B = 8, 2, 128, 3
    cos, sin = _tables(MAX_LEN, hd)
    q, k, v, kc, vc = _inputs(B, heads, kvh, hd, seed=5)
    ws = rope_attn_batched_workspace(B, heads, hd, DEV)
    good = torch.tensor([5, 7, 300], device=DEV)
    kg, vg = kc.clone(), vc.clone()
    out_good = torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, cos, sin, good, kg, vg, ws, 0)
    for _ in range(2):          # the sequences that did run leave the workspace reusable
        kb, vb = kc.clone(), vc.clone()
        out = torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, cos, sin, torch.tensor([5, bad, 300], device=DEV),
                                                          kb, vb, ws, 0)
        assert torch.isnan(out[1]).all()
        assert torch.equal(kb[1].view(torch.int16), kc[1].view(torch.int16))
        assert torch.equal(vb[1].view(torch.int16), vc[1].view(torch.int16))
        for b in (0, 2):
            assert torch.equal(out[b], out_good[b]) and torch.equal(kb[b], kg[b]) and torch.equal(vb[b], vg[b])


@pytest.mark.parametrize("n", [7, 32000, 128256])
def test_argmax_step_batched_matches_torch_per_row(n):
    """tok[b] = first index of the maximum of row b (ties), all-NaN / all -inf rows give 0, pos[b] += 1 once"""
    import quip_for_all_amd.batch_decode  # noqa: F401
    B = 6
    g = torch.Generator().manual_seed(n)
    logits = torch.randn(B, n, generator=g).half()
    logits[1, n // 3] = logits[1, n - 1] = 9.0           # a tie: the first index wins
    logits[1, 0] = 8.0
    logits[2] = float("nan")
    logits[3] = -float("inf")
    logits[4] = 0.0                                      # every entry tied
    logits = logits.to(DEV)
    tok = torch.full((B,), -5, dtype=torch.long, device=DEV)
    pos0 = torch.arange(B, dtype=torch.long, device=DEV) * 11
    pos = pos0.clone()
    torch.ops.quip_lib.argmax_step_batched(logits, tok, pos)
    want = torch.argmax(logits.float(), dim=-1)
    want[2] = want[3] = 0
    assert torch.equal(tok, want), (tok, want)
    assert int(tok[1]) == n // 3 and int(tok[4]) == 0
    assert torch.equal(pos, pos0 + 1)


def _prompts(vocab, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).to(DEV) for n in lengths]


def _bs1_forced(dec, prompt, forced):
    """logits (and pre-head states) of the bs=1 decoder over `prompt` and then the tokens `forced`, one step each"""
    cap = []
    head = dec._head
    dec._head = lambda h: (cap.append(h.clone()), head(h))[1]
    try:
        dec.reset(int(prompt[-1]))
        if prompt.numel() > 1:
            dec.prefill(prompt[:-1])
        out = []
        with torch.no_grad():
            for t in forced:
                out.append(dec.step()[0].clone())
                dec.tok.fill_(int(t))
    finally:
        del dec._head
    return out, cap


def _batched_forced(bd, prompts, forced):
    cap = []
    head = bd._head
    bd._head = lambda h: (cap.append(h.clone()), head(h))[1]
    try:
        bd.reset()
        for b, pr in enumerate(prompts):
            bd.fill_slot(b, pr)
        out = []
        with torch.no_grad():
            for t in range(forced.shape[1]):
                out.append(bd.step().clone())
                bd.tok.copy_(forced[:, t])
    finally:
        del bd._head
    return out, cap


def _exact_setup(shape_name, monkeypatch):
    from quip_for_all_amd import decode as D
    from quip_for_all_amd.qlinear import QuantLinear
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    np.random.seed(11)
    dec = D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=64, device=DEV, seed=3)
    dec.ffn_eng = dec.block_eng = dec.fused_prologue = False        # the bs=1 stage-wise step
    return dec


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_batched_decoder_equals_bs1_stagewise_decoder(shape_name, monkeypatch):
    """QuantLinear.skinny_exact: every product with digit planes takes rows_exact (bit identical to bs=1 per row; TINY's
    down_proj has none -- K = 43 on a 16-point transform -- and takes the codebook's own product at M = 1 and M = B
    alike); per sequence, the greedy tokens, the states that enter the head and the logits (torch's lm_head GEMM at
    M = B included) equal the bs=1 stage-wise decoder's bit for bit"""
    dec = _exact_setup(shape_name, monkeypatch)
    bd = dec.batched(4)
    regimes = bd.regimes()
    for name, r in regimes.items():
        m1 = dec.layers[0][name].regime(1)
        assert r == ("rows_exact" if m1 == "gemv_planes" else m1), (name, r, m1)
    prompts = _prompts(dec.s.vocab, (1, 5, 9, 17), seed=2)
    toks = bd.generate(prompts, 8)
    assert torch.equal(toks, bd.generate(prompts, 8, use_graph=False))
    for b, pr in enumerate(prompts):
        ref = dec.generate(8, prompt=pr, use_graph=False)
        assert torch.equal(toks[b], ref), (b, toks[b], ref)
    forced = torch.randint(0, dec.s.vocab, (4, 4), generator=torch.Generator().manual_seed(8)).to(DEV)
    lb, hb = _batched_forced(bd, prompts, forced)
    for b, pr in enumerate(prompts):
        l1, h1 = _bs1_forced(dec, pr, forced[b])
        for t in range(4):
            assert torch.equal(hb[t][b], h1[t][0]), (b, t, "state entering the head")
            assert torch.equal(lb[t][b], l1[t]), (b, t, "logits")


@pytest.mark.parametrize("kv_heads,ffn", [(32, 11008), (8, 14336)])
def test_batched_decoder_in_the_skinny_regime(kv_heads, ffn):
    """2-layer 4096-wide decoders, B = 8: every product takes the skinny fp16 kernel.  Teacher forced, each sequence's
    logits lie within 2 deep_bound_ulps(2) of the bs=1 decoder's; the greedy choice agrees except near ties; graph
    replay == eager step"""
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=4096, ffn=ffn, layers=2, heads=32, kv_heads=kv_heads, vocab=1024)
    np.random.seed(13)
    dec = D.LlamaDecoder(shape, "E8P12", max_len=32, device=DEV, seed=4, device_init=True)
    bd = dec.batched(8)
    assert set(bd.regimes().values()) == {"skinny_fp16"}, bd.regimes()
    prompts = _prompts(shape.vocab, (1, 2, 3, 4, 5, 6, 7, 8), seed=3)
    forced = torch.randint(0, shape.vocab, (8, 3), generator=torch.Generator().manual_seed(9)).to(DEV)
    lb, _ = _batched_forced(bd, prompts, forced)
    bound = 2 * deep_bound_ulps(2)
    worst = 0.0
    for b, pr in enumerate(prompts):
        l1, _ = _bs1_forced(dec, pr, forced[b])
        for t in range(3):
            got, ref = lb[t][b].double().cpu().numpy(), l1[t].double().cpu().numpy()
            u = _ulps_of_rms(got, ref)
            worst = max(worst, u)
            assert u <= bound, (b, t, u, bound)
            srt = np.sort(ref)
            assert int(np.argmax(got)) == int(np.argmax(ref)) or srt[-1] - srt[-2] < 0.05, (b, t)
    print(f"skinny regime, B = 8, kv_heads {kv_heads}: max {worst:.2f} fp16 ulps of rms(logits) (bound {bound:.1f})")
    toks = bd.generate(prompts, 4)
    graph_logits = bd.step_logits.clone()
    assert torch.equal(toks, bd.generate(prompts, 4, use_graph=False))
    assert torch.equal(graph_logits, bd.step_logits)


def test_refilling_one_slot_leaves_the_others_alone(monkeypatch):
    """continuous batching: slot 1 restarts on a new prompt mid-generation; the other slots' tokens and logits are
    bit identical to an uninterrupted run, slot 1 follows a fresh bs=1 run of the new prompt"""
    dec = _exact_setup("TINY", monkeypatch)
    bd = dec.batched(4)
    prompts = _prompts(dec.s.vocab, (3, 1, 6, 2), seed=4)
    new = _prompts(dec.s.vocab, (5,), seed=5)[0]

    def run(refill):
        bd.reset()
        for b, pr in enumerate(prompts):
            bd.fill_slot(b, pr)
        toks, lg = [], []
        with torch.no_grad():
            for t in range(8):
                if refill and t == 3:
                    bd.fill_slot(1, new)
                lg.append(bd.step().clone())
                toks.append(bd.tok.clone())
        return torch.stack(toks, 1), lg
    t_plain, l_plain = run(False)
    t_refill, l_refill = run(True)
    for b in (0, 2, 3):
        assert torch.equal(t_plain[b], t_refill[b])
        assert all(torch.equal(l_plain[t][b], l_refill[t][b]) for t in range(8))
    ref = dec.generate(5, prompt=new, use_graph=False)
    assert torch.equal(t_refill[1, 3:], ref), (t_refill[1, 3:], ref)
    l1, _ = _bs1_forced(dec, new, ref[:4])
    for t in range(4):
        assert torch.equal(l_refill[3 + t][1], l1[t]), t
