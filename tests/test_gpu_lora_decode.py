"""LoRA adapters on the decoders (TINY, E8P12, max_len 128; three adapters: r 8 on q, v; r 16 on all seven; r 4 with rsLoRA
on o, down): the float64 model with the adapters, bits kept without an adapter, captured steps that follow set_adapter,
chunked / ragged / paged / batched passes bit for bit, and the chain / prologue route on SMALL."""
import functools

import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from tests.test_gpu_decode import _TINY_ULPS, _params, _ulps_of_rms
from tests.test_lora_host import PEFT, config, make_adapter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN = 128
ALL = ("q", "k", "v", "o", "gate", "up", "down")
# name -> (r, targets, rsLoRA).  lora_alpha = 2 r (tests/test_lora_host.py: config), so scale = 2, or 2 sqrt(r) with rsLoRA.
ADAPTERS = {"qv8": (8, ("q", "v"), False), "all16": (16, ALL, False), "od4": (4, ("o", "down"), True)}
# Weight scale of the random adapters: A ~ AMP N(0, 1 / in), B ~ AMP N(0, 1), so |scale B A x| ~ scale AMP^2 sqrt(r) |x|:
# with AMP = 0.2 between 0.2 and 0.3 of the base module's |y| ~ |x| -- a fine-tune's order of magnitude.  Chosen with the
# float64 model below on the CPU (the oracle needs no GPU): at AMP = 0.2 the logits of step 3 with and without each adapter
# differ by 2286 (qv8), 4249 (all16) and 1359 (od4) fp16 ulps of rms(logits) on TINY and by 1951 (all16) on SMALL, against
# the 120 the materiality condition asks for; the condition is asserted on those float64 values in the tests below.
AMP = 0.2
FORCED = (5, 17, 40)          # teacher-forced tokens of the float64 comparison: one reference per adapter serves every route


def _dims(shape):
    kv = shape.kv_heads * shape.head_dim
    return {"q": (shape.hidden, shape.q_width), "k": (shape.hidden, kv), "v": (shape.hidden, kv),
            "o": (shape.q_width, shape.hidden), "gate": (shape.hidden, shape.ffn), "up": (shape.hidden, shape.ffn),
            "down": (shape.ffn, shape.hidden)}


@functools.lru_cache(maxsize=None)
def _adapter(shape_name, name):
    from quip_for_all_amd import decode as D
    shape = getattr(D, shape_name)
    r, targets, rs = ADAPTERS[name]
    seed = 100 + list(ADAPTERS).index(name)
    return make_adapter(_dims(shape), shape.layers, r, targets, seed=seed, amp=AMP), config(r, targets, use_rslora=rs)


def _build(shape_name="TINY", device=DEV, lora=True, max_len=MAX_LEN):
    from quip_for_all_amd import decode as D
    np.random.seed(11)
    dec = D.LlamaDecoder(getattr(D, shape_name), "E8P12", max_len=max_len, device=device, seed=3)
    if lora:
        dec.enable_lora(max_adapters=4, max_rank=16)
        for name in ADAPTERS:
            dec.load_adapter(name, *_adapter(shape_name, name))
    return dec


@functools.lru_cache(maxsize=None)
def _decoder(shape_name="TINY"):
    dec = _build(shape_name)
    assert dec.lora is not None and not dec.block_eng and not dec.ffn_eng and not dec.attn_z and not dec._token_tail_on()
    assert [dec.lora.index(n) for n in ADAPTERS] == [0, 1, 2]
    return dec


def _fresh(shape_name="TINY", adapter=None):
    dec = _decoder(shape_name)
    dec.reset()
    dec.kcache.zero_()
    dec.vcache.zero_()
    dec.set_adapter(adapter)
    return dec


def _bits(t):
    return t.contiguous().view(torch.int16)


def ref_logits(dec, tokens, shape_name, adapter):
    """tests/test_gpu_decode.py's float64 model with lin(name, x) + scale B (A x) for the modules `adapter` targets (the
    adapter's fp16 weights in float64; x: the float64 input of the base module)"""
    s = dec.s
    P = [{k: (_params(v) if hasattr(v, "Qidxs") else v.float().cpu().numpy().astype(np.float64))
          for k, v in L.items() if k != "lora"} for L in dec.layers]
    W = [{k: O.qlinear_dense_weight(p) for k, p in L.items() if isinstance(p, O.QLinearParams)} for L in P]
    emb = dec.embed.float().cpu().numpy().astype(np.float64)
    cos, sin = dec.cos.cpu().numpy().astype(np.float64), dec.sin.cpu().numpy().astype(np.float64)
    ad, scale = {}, 0.0
    if adapter is not None:
        from quip_for_all_amd.lora import check_config
        tensors, cfg = _adapter(shape_name, adapter)
        _, scale, targets = check_config(cfg, 16)
        for i in range(s.layers):
            for m in targets:
                ad[(i, m)] = tuple(tensors[f"base_model.model.model.layers.{i}.{PEFT[m]}.lora_{ab}.weight"].double().numpy()
                                   for ab in "AB")

    def rms(h, w):
        return h / np.sqrt((h * h).mean() + s.rms_eps) * w

    def rope(x, p):
        d = x.shape[-1] // 2
        rot = np.concatenate([-x[..., d:], x[..., :d]], -1)
        return x * cos[p] + rot * sin[p]
    ks = [[] for _ in P]
    vs = [[] for _ in P]
    for p, t in enumerate(tokens):
        h = emb[t]
        for i, L in enumerate(P):
            def lin(name, v):
                y = O.qlinear_forward(L[name], v[None], "exact", W[i][name])[0]
                if (i, name) in ad:
                    A, B = ad[(i, name)]
                    y = y + scale * (B @ (A @ v))
                return y
            x = rms(h, L["ln1"])
            q = rope(lin("q", x).reshape(s.heads, s.head_dim), p)
            k = rope(lin("k", x).reshape(s.kv_heads, s.head_dim), p)
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


@functools.lru_cache(maxsize=None)
def _refs(shape_name):
    """float64 logits of step 3 on FORCED, without an adapter and with each: computed once, shared, never changed"""
    dec = _decoder(shape_name)
    names = [None] + (list(ADAPTERS) if shape_name == "TINY" else ["all16"])
    return {a: ref_logits(dec, FORCED, shape_name, a) for a in names}


def _forced_logits(dec, adapter, n=len(FORCED)):
    """logits of the last of the eager steps over FORCED"""
    dec.reset(FORCED[0])
    dec.kcache.zero_()
    dec.vcache.zero_()
    dec.set_adapter(adapter)
    with torch.no_grad():
        for t in range(n):
            dec.tok.fill_(FORCED[t])
            logits = dec.step()
    return logits.float().cpu().numpy()[0].astype(np.float64)


@pytest.mark.parametrize("name", list(ADAPTERS))
def test_float64_model_with_adapters(name):
    """logits of step 3 within the bound the plain TINY E8P12 decoder is held to (12 fp16 ulps of rms(logits): the adapter
    path adds one fp16 rounding per module, its fp32 delta is more exact than the base product); observed values:
    profiles/lora_model_ulps.txt.  Materiality, on the float64 values: the adapter moves the logits by at least 10 x
    that bound -- a decoder that ignored it would fail."""
    dec = _fresh()
    refs = _refs("TINY")
    ref, base = refs[name], refs[None]
    moved = _ulps_of_rms(base, ref)
    assert moved >= 10 * _TINY_ULPS["E8P12"], (name, moved)
    try:
        for fused in ((True, False) if dec.fused_prologue else (False,)):         # both bs = 1 routes where there are two
            dec.lora_fused_step, dec.graph = fused, None
            u = _ulps_of_rms(_forced_logits(dec, name), ref)
            u0 = _ulps_of_rms(_forced_logits(dec, None), base)
            print(f"LoRA decoder TINY E8P12, adapter {name}, {'_step_fused' if fused else '_block'}: logits of step 3 vs float64: "
                  f"max {u:.2f} fp16 ulps of rms (no adapter: {u0:.2f}; the adapter moves the float64 logits by {moved:.0f})")
            assert u <= _TINY_ULPS["E8P12"], (fused, u)
            assert u0 <= _TINY_ULPS["E8P12"], (fused, u0)
    finally:
        dec.lora_fused_step, dec.graph = True, None
        dec.set_adapter(None)


def _steps(dec, n, first=7):
    dec.reset(first)
    dec.kcache.zero_()
    dec.vcache.zero_()
    out = []
    with torch.no_grad():
        for _ in range(n):
            out.append(dec.step().clone())
    return out, dec.kcache.clone(), dec.vcache.clone()


def test_enable_lora_without_an_adapter_keeps_every_bit():
    """logits and caches of 8 steps: the decoder before enable_lora == after it == with three adapters loaded and none
    selected == selected and unloaded again"""
    dec = _build(lora=False)
    assert dec.lora is None
    want = _steps(dec, 8)
    dec.enable_lora(max_adapters=4, max_rank=16)
    assert not dec.block_eng and not dec.ffn_eng and not dec.attn_z and dec.graph is None

    def same(got):
        return all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got[0], want[0])) and \
            torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert same(_steps(dec, 8))
    for name in ADAPTERS:
        dec.load_adapter(name, *_adapter("TINY", name))
    assert same(_steps(dec, 8))
    dec.set_adapter("all16")
    assert not same(_steps(dec, 8))
    dec.set_adapter(None)
    assert same(_steps(dec, 8))
    # a re-run of the runtime set-up keeps the adapter state and the switches
    lora = dec.lora
    dec._init_runtime()
    assert dec.lora is lora and not dec.block_eng and not dec.ffn_eng and not dec.attn_z and dec.layers[0]["lora"] is lora.layers[0]
    assert same(_steps(dec, 8))
    with pytest.raises(RuntimeError, match="already"):
        dec.enable_lora()
    with pytest.raises(KeyError):
        dec.set_adapter("nobody")


def test_captured_step_equals_eager_and_follows_set_adapter():
    """captured == eager tokens per adapter; the adapter switched between replays WITHOUT a new capture gives the eager
    run's tokens of the new adapter; so does an adapter loaded into a free slot after the capture"""
    dec = _fresh()
    eager = {}
    for name in [None] + list(ADAPTERS):
        dec.set_adapter(name)
        eager[name] = dec.generate(12, first_token=5, use_graph=False)
    assert len({tuple(t.tolist()) for t in eager.values()}) > 1            # (the adapters change the tokens)
    dec.set_adapter("qv8")
    assert torch.equal(dec.generate(12, first_token=5, use_graph=True), eager["qv8"])
    graph = dec.graph
    assert graph is not None
    for name in ("all16", None, "od4", "qv8"):
        dec.set_adapter(name)
        assert torch.equal(dec.generate(12, first_token=5, use_graph=True), eager[name]), name
        assert dec.graph is graph
    # a fourth adapter, same targets as loaded ones: the captured step stays and serves it
    r, targets = 8, ("q", "v", "down")
    extra = make_adapter(_dims(dec.s), dec.s.layers, r, targets, seed=77, amp=AMP)
    try:
        assert dec.load_adapter("extra", extra, config(r, targets)) == 3 and dec.graph is graph
        dec.set_adapter("extra")
        want = dec.generate(12, first_token=5, use_graph=False)
        assert torch.equal(dec.generate(12, first_token=5, use_graph=True), want) and dec.graph is graph
        assert not torch.equal(want, eager[None])
    finally:
        dec.unload_adapter("extra")
        dec.set_adapter(None)


def test_extend_in_chunks_keeps_bits_and_score_runs(monkeypatch):
    """QuantLinear.skinny_exact (every product bit identical to bs = 1 per row, the project's condition for this statement):
    extend in chunks of 1, 3 and all at once leaves the same cache rows and returns the same logits, with and without an
    adapter; score / perplexity run and see the adapter"""
    from quip_for_all_amd.qlinear import QuantLinear
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    dec = _fresh()
    toks = torch.randint(0, dec.s.vocab, (11,), generator=torch.Generator().manual_seed(4)).to(DEV)
    got = {}
    for name in (None, "all16"):
        for chunk in (1, 3, 512):
            dec = _fresh(adapter=name)
            with torch.no_grad():
                lg = dec.extend(toks, chunk=chunk)
            got[(name, chunk)] = (lg.clone(), dec.kcache.clone(), dec.vcache.clone())
            assert int(dec.pos) == 11
        for chunk in (1, 3):
            for a, b in zip(got[(name, chunk)], got[(name, 512)]):
                assert torch.equal(_bits(a), _bits(b)), (name, chunk)
    assert not torch.equal(got[(None, 512)][0], got[("all16", 512)][0])
    lps = {}
    for name in (None, "od4"):
        dec = _fresh(adapter=name)
        lp, am = dec.score(toks, chunk=4)
        assert tuple(lp.shape) == (11,) and bool(torch.isfinite(lp).all()) and float(lp[-1]) == 0.0
        lps[name] = lp
        ppl = dec.perplexity(toks, window=8, stride=4, chunk=3)
        assert ppl["n_scored"] == 10 and np.isfinite(ppl["ppl"])
    assert not torch.equal(lps[None], lps["od4"])
    dec.set_adapter(None)


SLOT_ADAPTERS = ["qv8", "all16", None, "od4", "all16"]          # indices [0, 1, -1, 2, 1]


def _prompts(vocab, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=g).to(DEV) for n in lengths]


def _run_batch(bd, prompts, names, steps=4):
    """fill_slots (the ragged pass) + `steps` eager steps -> (logits per step, positions)"""
    bd.reset()
    for b, n in enumerate(names):
        bd.set_slot_adapter(b, n)
    with torch.no_grad():
        bd.fill_slots(range(bd.batch), prompts)
        if hasattr(bd, "pool"):          # (a paged cache: the pages of the steps, as PagedBatchDecoder.decode reserves them)
            bd._assign({b: bd.pool.length[b] + steps for b in range(bd.batch)})
        out = [bd.step().clone() for _ in range(steps)]
    return out, bd.pos.clone()


@pytest.mark.parametrize("paged", [False, True])
def test_mixed_adapters_in_one_batch(paged):
    """B = 5, adapters [0, 1, -1, 2, 1]: every slot's logits equal, bit for bit, those of the same batch with that slot's
    adapter on ALL slots (prompt pass and steps); the slot tensor holds the indices; reset() keeps them"""
    dec = _fresh()
    bd = dec.batched(5, max_len=64, paged=paged)
    prompts = _prompts(dec.s.vocab, (1, 5, 9, 17, 3), seed=2)
    mixed, _ = _run_batch(bd, prompts, SLOT_ADAPTERS)
    assert bd.slot_adapter.tolist() == [0, 1, -1, 2, 1]
    bd.reset()
    assert bd.slot_adapter.tolist() == [0, 1, -1, 2, 1]
    rows = {}
    for name in set(SLOT_ADAPTERS):
        uniform, _ = _run_batch(bd, prompts, [name] * 5)
        rows[name] = uniform
        for b, n in enumerate(SLOT_ADAPTERS):
            if n == name:
                for t in range(len(mixed)):
                    assert torch.equal(_bits(mixed[t][b]), _bits(uniform[t][b])), (name, b, t)
    assert not torch.equal(rows[None][-1], rows["all16"][-1]) and not torch.equal(rows["qv8"][-1], rows["od4"][-1])
    with pytest.raises(KeyError):
        bd.set_slot_adapter(0, "nobody")
    with pytest.raises(ValueError):
        bd.set_slot_adapter(5, None)


def test_paged_equals_contiguous_and_a_fork_takes_its_sources_adapter():
    dec = _fresh()
    prompts = _prompts(dec.s.vocab, (1, 5, 9, 17, 3), seed=3)
    cont, pos_c = _run_batch(dec.batched(5, max_len=64), prompts, SLOT_ADAPTERS)
    pd = dec.batched(5, max_len=64, paged=True)
    paged, pos_p = _run_batch(pd, prompts, SLOT_ADAPTERS)
    assert torch.equal(pos_c, pos_p)
    for a, b in zip(cont, paged):
        assert torch.equal(_bits(a), _bits(b))
    # slot 2 (no adapter) becomes a fork of slot 1 (all16): it continues like its source
    pd.fork_slot(1, 2)
    assert pd.slot_adapter.tolist() == [0, 1, 1, 2, 1]
    pd._assign({b: pd.pool.length[b] + 3 for b in range(5)})
    with torch.no_grad():
        for _ in range(3):
            lg = pd.step()
            assert torch.equal(_bits(lg[2]), _bits(lg[1])) and not torch.equal(_bits(lg[2]), _bits(lg[4]))
    pd.free_slot(2)
    assert pd.slot_adapter.tolist() == [0, 1, -1, 2, 1]


def test_extend_slots_equals_extend_slot_one_by_one(monkeypatch):
    """slots with different adapters through ONE ragged pass == each slot through its own chunked pass: logits and caches
    (QuantLinear.skinny_exact: the passes differ in their row counts)"""
    from quip_for_all_amd.qlinear import QuantLinear
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    dec = _fresh()
    lists = _prompts(dec.s.vocab, (7, 1, 12, 4), seed=6)
    slots = [3, 0, 1, 2]
    a, b = dec.batched(5, max_len=64), dec.batched(5, max_len=64)
    for bd in (a, b):
        for s_, n in enumerate(SLOT_ADAPTERS):
            bd.set_slot_adapter(s_, n)
    with torch.no_grad():
        la = a.extend_slots(slots, lists, chunk=5)
        lb = torch.cat([b.extend_slot(s_, t, chunk=5) for s_, t in zip(slots, lists)])
    assert torch.equal(_bits(la), _bits(lb))
    assert torch.equal(a.kcache, b.kcache) and torch.equal(a.vcache, b.vcache) and torch.equal(a.pos, b.pos)
    # and the adapters were in it: slot 1 (all16) differs from the same tokens without an adapter
    c = dec.batched(5, max_len=64)
    with torch.no_grad():
        lc = c.extend_slot(1, lists[2], chunk=5)
    assert not torch.equal(_bits(lc[0]), _bits(la[2]))


def test_batched_slot_equals_the_bs1_block_route(monkeypatch):
    """the conditions of tests/test_gpu_batch_decode.py::test_batched_decoder_equals_bs1_stagewise_decoder
    (QuantLinear.skinny_exact: every product with digit planes is bit identical per row): per slot the greedy tokens equal
    the bs = 1 decoder's on the _block route with that slot's adapter; captured == eager"""
    from quip_for_all_amd.qlinear import QuantLinear
    monkeypatch.setattr(QuantLinear, "skinny_exact", True)
    dec = _fresh()
    names = SLOT_ADAPTERS[:4]
    bd = dec.batched(4, max_len=64)
    for b, n in enumerate(names):
        bd.set_slot_adapter(b, n)
    prompts = _prompts(dec.s.vocab, (1, 5, 9, 17), seed=2)
    toks = bd.generate(prompts, 8)
    assert torch.equal(toks, bd.generate(prompts, 8, use_graph=False))
    dec.lora_fused_step, dec.graph = False, None          # the bs = 1 _block route
    try:
        for b, pr in enumerate(prompts):
            dec.set_adapter(names[b])
            ref = dec.generate(8, prompt=pr, use_graph=False)
            assert torch.equal(toks[b], ref), (b, names[b], toks[b], ref)
    finally:
        dec.lora_fused_step, dec.graph = True, None
        dec.set_adapter(None)


def test_chain_route_with_adapters_on_small():
    """SMALL takes the chain / GEMV-prologue step: with lora_fused_step the hooks of _step_fused carry the adapter -- within
    the float64 model's bound, the adapter material, captured == eager; the persistent launches, ffn_eng and attn_z are
    off; it is the default bs = 1 route with adapters (profiles/lora_bench.txt), _block the other"""
    dec = _decoder("SMALL")
    assert dec.fused_prologue and not dec.block_eng and not dec.ffn_eng and not dec.attn_z and not dec._token_tail_on()
    assert dec.lora_fused_step
    refs = _refs("SMALL")
    moved = _ulps_of_rms(refs[None], refs["all16"])
    assert moved >= 10 * _TINY_ULPS["E8P12"], moved
    try:
        for fused in (False, True):
            dec.lora_fused_step, dec.graph = fused, None
            u = _ulps_of_rms(_forced_logits(dec, "all16"), refs["all16"])
            u0 = _ulps_of_rms(_forced_logits(dec, None), refs[None])
            print(f"LoRA decoder SMALL E8P12, adapter all16, {'_step_fused' if fused else '_block'}: logits of step 3 vs float64: "
                  f"max {u:.2f} fp16 ulps of rms (no adapter: {u0:.2f}; the adapter moves the float64 logits by {moved:.0f})")
            assert u <= _TINY_ULPS["E8P12"], (fused, u)
        assert dec.lora_fused_step
        dec.set_adapter("all16")
        eager = dec.generate(10, first_token=7, use_graph=False)
        assert torch.equal(dec.generate(10, first_token=7, use_graph=True), eager)
        graph = dec.graph
        dec.set_adapter(None)
        plain = dec.generate(10, first_token=7, use_graph=True)
        assert dec.graph is graph and not torch.equal(plain, eager)
    finally:
        dec.lora_fused_step, dec.graph = True, None
        dec.set_adapter(None)
