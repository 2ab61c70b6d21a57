"""Decoders on models with per-head q / k RMSNorm and a free head_dim (Qwen3; random init, `LlamaDecoder(qk_norm=True)`):
the float64 model, and the equivalence of the routes -- fused against stand-alone norm launch, chunked extend, contiguous
against paged, forked slots, batched against bs = 1 -- bit for bit where the project holds Llama models to bits."""
import functools

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from tests.test_gpu_decode import _TINY_ULPS, _params, _ulps_of_rms

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 128
MODELS = ["HD128", "HD64"]


def _shape(name):
    from quip_for_all_amd import decode as D
    return {"HD128": D.LlamaShape(hidden=256, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512, head_dim=128),
            "HD64": D.TINY}[name]


@functools.lru_cache(maxsize=None)
def _decoder(name):
    from quip_for_all_amd import decode as D
    np.random.seed(11)
    dec = D.LlamaDecoder(_shape(name), "E8P12", max_len=MAX_LEN, device=DEV, seed=3, qk_norm=True)
    assert dec.qk_norm and dec.qk_fused and not dec.block_eng and not dec.attn_z and not dec._token_tail_on()
    return dec


def _fresh(name):
    dec = _decoder(name)
    dec.reset()
    dec.kcache.zero_()
    dec.vcache.zero_()
    return dec


def _tokens(dec, n, seed):
    return torch.randint(0, dec.s.vocab, (n,), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ref_logits(dec, tokens):
    """tests/test_gpu_decode.py's float64 model with the q / k norm in float64 and the free head_dim"""
    s = dec.s
    P = [{k: (_params(v) if hasattr(v, "Qidxs") else v.float().cpu().numpy().astype(np.float64))
          for k, v in L.items()} for L in dec.layers]
    W = [{k: O.qlinear_dense_weight(p) for k, p in L.items() if isinstance(p, O.QLinearParams)} for L in P]
    emb = dec.embed.float().cpu().numpy().astype(np.float64)
    cos, sin = dec.cos.cpu().numpy().astype(np.float64), dec.sin.cpu().numpy().astype(np.float64)

    def rms(h, w, eps=s.rms_eps):
        return h / np.sqrt((h * h).mean(-1, keepdims=True) + eps) * w

    def rope(x, p):
        d = x.shape[-1] // 2
        rot = np.concatenate([-x[..., d:], x[..., :d]], -1)
        return x * cos[p] + rot * sin[p]
    ks = [[] for _ in P]
    vs = [[] for _ in P]
    for p, t in enumerate(tokens):
        h = emb[t]
        for i, L in enumerate(P):
            x = rms(h, L["ln1"])
            lin = lambda name, v: O.qlinear_forward(L[name], v[None], "exact", W[i][name])[0]  # noqa: E731
            q = rope(rms(lin("q", x).reshape(s.heads, s.head_dim), L["q_norm"], dec.qk_eps), p)
            k = rope(rms(lin("k", x).reshape(s.kv_heads, s.head_dim), L["k_norm"], dec.qk_eps), p)
            v = lin("v", x).reshape(s.kv_heads, s.head_dim)
            ks[i].append(k)
            vs[i].append(v)
            K, V = np.stack(ks[i], 1), np.stack(vs[i], 1)          # (kv, T, d)
            rep = s.heads // s.kv_heads
            out = np.empty((s.heads, s.head_dim))
            for hh in range(s.heads):
                sc = K[hh // rep] @ q[hh] / np.sqrt(s.head_dim)
                w = np.exp(sc - sc.max())
                out[hh] = (w / w.sum()) @ V[hh // rep]
            h = h + lin("o", out.reshape(-1))
            x = rms(h, L["ln2"])
            gte = lin("gate", x)
            h = h + lin("down", gte / (1 + np.exp(-gte)) * lin("up", x))
        logits = rms(h, dec.final_norm.float().cpu().numpy().astype(np.float64)) @ \
            dec.lm_head.float().cpu().numpy().astype(np.float64).T
    return logits


@pytest.mark.parametrize("name", MODELS)
def test_decode_against_float64_model(name):
    """captured == eager tokens; logits of step 3 within the bound the plain TINY E8P12 decoder is held to (12 fp16 ulps of
    rms(logits)); the observed values are in profiles/qk_norm_model_ulps.txt"""
    dec = _fresh(name)
    eager = dec.generate(12, first_token=5, use_graph=False).cpu().numpy()
    graph = dec.generate(12, first_token=5, use_graph=True).cpu().numpy()
    np.testing.assert_array_equal(eager, graph)
    dec.reset(5)
    with torch.no_grad():
        for _ in range(3):
            logits = dec.step()
    ref = _ref_logits(dec, [5, int(eager[0]), int(eager[1])])
    got = logits.float().cpu().numpy()[0].astype(np.float64)
    u = _ulps_of_rms(got, ref)
    print(f"qk-norm decoder {name} (head_dim {dec.s.head_dim}, E8P12), logits of step 3 vs float64: max {u:.2f} fp16 ulps of rms")
    assert u <= _TINY_ULPS["E8P12"], u
    assert int(np.argmax(ref)) == int(eager[2]) or np.sort(ref)[-1] - np.sort(ref)[-2] < 0.05


def _steps(dec, n, first=7):
    dec.reset(first)
    dec.kcache.zero_()
    dec.vcache.zero_()
    out = []
    with torch.no_grad():
        for _ in range(n):
            out.append(dec.step().clone())
    return out, dec.kcache.clone(), dec.vcache.clone()


@pytest.mark.parametrize("name", MODELS)
def test_fused_step_equals_the_norm_launch_in_front(name):
    """the switch of tools/qk_norm_bench.py: qk_fused off runs quip_lib::qk_norm_rows in front of the plain attention launch
    -- logits and caches of 6 steps bit for bit, on the step the decoder takes by default and on the stage-wise one, and
    through the captured step"""
    dec = _fresh(name)
    keep = dec.fused_prologue
    try:
        for prologue in sorted({keep, False}):
            dec.fused_prologue = prologue
            dec.qk_fused = True
            a = _steps(dec, 6)
            dec.qk_fused = False
            b = _steps(dec, 6)
            for x, y in zip(a[0], b[0]):
                assert torch.equal(_bits(x), _bits(y)), prologue
            assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), prologue
            assert bool(torch.isfinite(a[0][-1]).all()) and bool(a[1][:, :, :6].any())
        dec.fused_prologue = keep
        toks = []
        for fused in (True, False):
            dec.qk_fused, dec.graph = fused, None
            toks.append(dec.generate(10, first_token=5, use_graph=True))
        assert torch.equal(toks[0], toks[1])
    finally:
        dec.fused_prologue, dec.qk_fused, dec.graph = keep, True, None


@pytest.mark.parametrize("name", MODELS)
def test_extend_chunks_give_the_same_bits(name, monkeypatch):
    """QuantLinear.skinny_exact (every product bit identical to bs = 1 per row): extend in chunks of 1, 3 and all at once
    leaves the same cache rows and returns the same logits; extend_graph replays them"""
    from quip_for_all_amd.qlinear import QuantLinear
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    toks = _tokens(_decoder(name), 10, 4)
    runs = []
    for chunk in (1, 3, 512):
        dec = _fresh(name)
        lg = dec.extend(toks, chunk=chunk)
        assert int(dec.pos) == 10
        runs.append((lg.clone(), dec.kcache.clone(), dec.vcache.clone()))
    for lg, kc, vc in runs[1:]:
        assert torch.equal(_bits(lg), _bits(runs[0][0])) and torch.equal(kc, runs[0][1]) and torch.equal(vc, runs[0][2])
    assert bool(torch.isfinite(runs[0][0]).all()) and not runs[0][1][:, :, 10:].any()
    dec = _fresh(name)
    lg = dec.extend_graph(toks)
    assert torch.equal(_bits(lg), _bits(runs[0][0])) and torch.equal(dec.kcache, runs[0][1])


@pytest.mark.parametrize("name", MODELS)
def test_prompt_routes_and_scores(name):
    """prefill (SDPA), extend (chunk launch) and token-by-token steps agree within the project's tolerance for equivalent
    routes, 0.03 (max|ref| + 1); score / perplexity / generate(append=True) run on such a model"""
    dec = _fresh(name)
    toks = _tokens(dec, 19, 7)
    lp = dec.prefill(toks).float().clone()
    kp = dec.kcache.clone()
    dec = _fresh(name)
    le = dec.extend(toks).float()
    tol = 0.03 * (float(lp.abs().max()) + 1.0)
    assert float((le - lp).abs().max()) <= tol
    assert torch.equal(dec.kcache[0][:, :19], kp[0][:, :19])       # block 0: same projections, same norm, same rotation
    dec = _fresh(name)
    with torch.no_grad():
        for t in range(19):
            dec.tok.copy_(toks[t:t + 1])
            ls = dec.step().float().clone()
    assert float((ls - lp).abs().max()) <= tol
    dec = _fresh(name)
    lps, am = dec.score(toks)
    assert tuple(lps.shape) == (19,) and bool(torch.isfinite(lps).all()) and float(lps[-1]) == 0.0 and bool((lps[:-1] < 0).all())
    r = dec.perplexity(toks, window=16, stride=8)
    assert r["n_scored"] == 18 and np.isfinite(r["ppl"])
    out = dec.generate(4, prompt=toks[:6], use_graph=False)
    out2 = dec.generate(3, prompt=toks[6:9], append=True)
    assert out.numel() == 4 and out2.numel() == 3 and dec._fed == 6 - 1 + 4 + 3 + 3


def _pair(name, pages=12):
    dec = _decoder(name)
    return dec, dec.batched(3), dec.batched(3, paged=True, pages=pages)


@pytest.mark.parametrize("name", MODELS)
def test_contiguous_and_paged_batches_give_the_same_bits(name):
    """fused norm (contiguous) against the norm launch in front of the paged launches: fill, chunked extend, scores,
    captured and eager decode"""
    dec, cont, paged = _pair(name)
    prompts = [_tokens(dec, n, 10 + n) for n in (63, 70, 5)]
    more = [_tokens(dec, 20, 20), _tokens(dec, 9, 21)]
    for d in (cont, paged):
        d.capture()
        d.fill_slots(range(3), prompts)
    le = [d.extend_slots([0, 2], more, chunk=16) for d in (cont, paged)]
    assert torch.equal(_bits(le[0]), _bits(le[1]))
    sc = [d.score_slots([1], [_tokens(dec, 6, 22)]) for d in (cont, paged)]
    assert torch.equal(sc[0][0][0], sc[1][0][0]) and torch.equal(sc[0][1][0], sc[1][1][0]) and bool(torch.isfinite(sc[0][0][0]).all())
    for use_graph in (True, False):
        for _ in range(3):
            for d in (cont, paged):
                d.decode(1, use_graph=use_graph)
            assert torch.equal(_bits(cont.step_logits), _bits(paged.step_logits)), use_graph
            assert torch.equal(cont.tok, paged.tok) and torch.equal(cont.pos, paged.pos)
    assert bool(torch.isfinite(cont.step_logits).all())
    for b in range(3):
        n = int(cont.pos[b])
        k, v = paged.gather_slot(b)
        assert torch.equal(k, cont.kcache[:, b, :, :n]) and torch.equal(v, cont.vcache[:, b, :, :n]), b
    toks = [d.generate(prompts, 4) for d in (cont, paged)]
    assert torch.equal(toks[0], toks[1])
    assert tuple(cont.generate(prompts, 4, ragged=True).shape) == (3, 4)


@pytest.mark.parametrize("name", MODELS)
def test_forked_slot_shares_the_prefix_and_continues_like_its_source(name):
    dec, _, paged = _pair(name)
    paged.reset()
    paged.fill_slots([0], [_tokens(dec, 70, 31)])
    free = paged.pages_free()
    paged.fork_slot(0, 2)
    assert paged.pool.table[2][0] == paged.pool.table[0][0] and paged.pool.table[2][1] != paged.pool.table[0][1]
    assert paged.pages_free() == free - 1 and paged.pool.check()
    paged.fill_slots([1], [_tokens(dec, 3, 32)])
    with torch.no_grad():
        for _ in range(3):
            paged.decode(1, use_graph=False)
            assert torch.equal(_bits(paged.step_logits[0]), _bits(paged.step_logits[2]))
            assert int(paged.tok[0]) == int(paged.tok[2])
    k0, v0 = paged.gather_slot(0)
    k2, v2 = paged.gather_slot(2)
    assert torch.equal(k0, k2) and torch.equal(v0, v2) and k0.shape[2] == 72


@pytest.mark.parametrize("name", MODELS)
def test_batched_decoder_equals_bs1_stagewise_decoder(name, monkeypatch):
    """tests/test_gpu_batch_decode.py's statement for Llama, on a q / k norm model: QuantLinear.skinny_exact, per sequence
    the greedy tokens, the states that enter the head and the logits equal the bs = 1 stage-wise decoder's bit for bit"""
    from quip_for_all_amd.qlinear import QuantLinear
    from tests.test_gpu_batch_decode import _batched_forced, _bs1_forced, _prompts
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    dec = _fresh(name)
    keep = (dec.ffn_eng, dec.block_eng, dec.fused_prologue)
    dec.ffn_eng = dec.block_eng = dec.fused_prologue = False        # the bs=1 stage-wise step
    try:
        bd = dec.batched(4, max_len=64)
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
    finally:
        dec.ffn_eng, dec.block_eng, dec.fused_prologue = keep
        dec.graph = None


@pytest.mark.parametrize("name", MODELS)
def test_fp8_paged_and_padded_decoders_follow_their_counterparts(name):
    """fp8 paged against fp16 paged, teacher forced: inside the bound tests/test_gpu_fp8_paged_decode.py holds TINY to;
    padded=True with start 0 (the norm launch in front of the padded-start launch) against the plain batched decoder
    (fused): bit for bit, as tests/test_gpu_batch_decode_padded.py states it; shifted rows: its 0.03 (max|ref| + 1)"""
    from tests.test_gpu_batch_decode_padded import _filled, _load
    from tests.test_gpu_fp8_paged_decode import _OBSERVED
    dec = _decoder(name)
    prompts = [_tokens(dec, n, 40 + n) for n in (5, 9, 17)]
    ref, f8 = dec.batched(3, paged=True, pages=9), dec.batched(3, paged=True, pages=9, kv_dtype="fp8")
    for d in (ref, f8):
        d.fill_slots(range(3), prompts)
    worst = 0.0
    for _ in range(4):
        f8.tok.copy_(ref.tok)
        for d in (ref, f8):
            d.decode(1, use_graph=False)
        assert bool(torch.isfinite(f8.step_logits).all())
        for x, y in zip(f8.step_logits.double().cpu().numpy(), ref.step_logits.double().cpu().numpy()):
            worst = max(worst, _ulps_of_rms(x, y))
    print(f"qk-norm {name}: fp8 paged vs fp16 paged logits: max {worst:.2f} fp16 ulps of rms(logits)")
    assert worst <= 2 * _OBSERVED[("TINY", "default")], worst
    plain, padded = dec.batched(3, max_len=64), dec.batched(3, max_len=64, padded=True)
    assert plain._fuses_norm() and not padded._fuses_norm()
    snap = _filled(plain, prompts)
    for bd in (plain, padded):
        _load(bd, snap)
    with torch.no_grad():
        for t in range(4):
            la, lb = plain.step(), padded.step()
            assert torch.equal(_bits(la), _bits(lb)), t
            assert torch.equal(plain.tok, padded.tok)
    assert torch.equal(_bits(plain.kcache), _bits(padded.kcache))
    starts = (0, 3, 11)
    _load(plain, snap)
    _load(padded, snap, starts)
    forced = torch.randint(0, dec.s.vocab, (3, 4), generator=torch.Generator().manual_seed(8)).to(DEV)
    with torch.no_grad():
        for t in range(4):
            r, g = plain.step().float(), padded.step().float()
            assert bool(torch.isfinite(g).all())
            for b in range(3):
                assert (g[b] - r[b]).abs().max().item() <= 0.03 * (r[b].abs().max().item() + 1.0), (t, b)
            for bd in (plain, padded):
                bd.tok.copy_(forced[:, t])


def test_persistent_launches_stay_off_on_a_qk_norm_model():
    """Llama-3-8B's block dims, 2 layers: without the norm this shape takes the persistent launch with the token tail; with
    it block_eng, attn_z and the token tail are off (they have no norm) and the stage-wise step decodes"""
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=4096, ffn=14336, layers=2, heads=32, kv_heads=8, vocab=1024)
    np.random.seed(23)
    dec = D.LlamaDecoder(shape, "E8P12", max_len=32, device=DEV, seed=9, device_init=True, qk_norm=True)
    assert dec.qk_norm and not dec.block_eng and not dec.attn_z and not dec._token_tail_on() and dec.eng_layers is None
    assert dec.fused_prologue                                   # (the 8-launch step, with the fused attention launch)
    toks = dec.generate(5, first_token=9, use_graph=True)
    assert bool(torch.isfinite(dec.step_logits).all())
    assert torch.equal(toks, dec.generate(5, first_token=9, use_graph=False))
    dec.qk_fused, dec.graph = False, None
    assert torch.equal(toks, dec.generate(5, first_token=9, use_graph=True))
