"""The Hadamard chain launch for hidden sizes K x 2^m with K = 3, 5, 7 (Llama-2-13B: 5120 = 5 x 1024; Qwen2-7B: 3584 =
7 x 512; Llama-3.2-3B: 3072 = 3 x 1024): one launch finishes the producer module (output transform + residual) and
starts its 1..3 consumers (RMSNorm, SU, input transform -> digit planes).  The bar is DESIGN section 2's: bit identical
to the launches it replaces -- h, every byte of every plane image, hence the GEMV outputs and the decoder's tokens."""
import numpy as np
import pytest
import torch

from oracle import quip_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _layer(P):
    import quip_for_all_amd as Q
    return Q.QuantLinear.from_params(P).to(DEV).eval()


def _t(a):
    return torch.from_numpy(np.asarray(a).astype(np.float16)).to(DEV)


def _separate(layers, prev, z, res, w):
    """the launches the chain replaces: prev's output transform, then the consumers' grouped planes launch"""
    from quip_for_all_amd import qlinear as QL
    l0 = layers[0]
    n, K = l0.q_in_features, l0.K_left
    (h,) = QL.out_transform_group([prev], [z], residual=[res])
    planes = torch.ops.quip_lib.had_transform_planes_group(
        h, n, K, [l._had("had_left") for l in layers], True, [l._vec(l.SU) for l in layers],
        [l.wscale_float / np.sqrt(n // K) for l in layers], w, 1e-5, None, getattr(l0.codebook, "planes_resid_scale", 0.0))
    return h, list(planes)


def _check_chain(cbid, k, fouts, with_rms, with_res, z=None):
    from quip_for_all_amd import qlinear as QL
    layers = [_layer(O.make_layer(cbid, k, fo, seed=k + fo + i)) for i, fo in enumerate(fouts)]
    prev = _layer(O.make_layer(cbid, 512, k, seed=k + 11))
    assert layers[0].K_left > 1 and prev.K_right == layers[0].K_left
    assert QL.chain_supported(layers, prev)
    rng = np.random.default_rng(k + len(fouts))
    w = _t(1 + 0.1 * rng.standard_normal(k)) if with_rms else None
    z = _t(rng.standard_normal((1, k)) * 8) if z is None else z
    res = _t(rng.standard_normal((1, k))) if with_res else None
    with torch.no_grad():
        h_ref, planes_ref = _separate(layers, prev, z, res, w)
        h, planes = QL.chain_planes(layers, prev, z, residual=res, rms_weight=w)
        h2, zs = QL.gemv_chain(layers, prev, z, residual=res, rms_weight=w)
        torch.cuda.synchronize()
        # bit patterns: a row that is not finite holds NaNs
        assert torch.equal(h.view(torch.int16), h_ref.view(torch.int16))
        assert torch.equal(h2.view(torch.int16), h_ref.view(torch.int16))
        assert len(planes) == len(planes_ref) == len(layers)
        for l, pl, pr, zf in zip(layers, planes, planes_ref, zs):
            assert pl.dtype == torch.uint8 and pl.shape == pr.shape
            # the image: three digit planes with their zeroed k padding, then the int32 shift word; the 12 bytes that
            # round the word up to 16 are written by no launch (torch.empty), so they are not compared
            used = pl.numel() - 12
            assert torch.equal(pl[:used], pr[:used])
            y = l.codebook.mm_planes(pr, l.Qidxs)
            assert torch.equal(zf.view(torch.int16), y.view(torch.int16))
    return h, planes


WIDTHS = [(5120, (5120, 5120, 5120)), (5120, (13824, 13824)), (3584, (3584, 512, 512)), (3072, (3072, 1024, 1024)),
          (1536, (1536,)), (7168, (7168,))]


@pytest.mark.parametrize("with_rms,with_res", [(True, True), (False, False), (True, False), (False, True)])
@pytest.mark.parametrize("k,fouts", WIDTHS)
def test_gemv_chain_k_bit_identical(k, fouts, with_rms, with_res):
    _check_chain("E8P12", k, fouts, with_rms, with_res)


@pytest.mark.parametrize("k,fouts", [(3 * 4096, (512,)), (5 * 2048, (1024, 512)), (7 * 2048, (512,)), (2560, (512, 512, 512)),
                                     (6144, (1024, 512))])
def test_gemv_chain_k_bit_identical_on_the_rest_of_the_range(k, fouts):
    """the ends of the range: L = 4096 (768 threads, the largest LDS image), 2048, n = 14336"""
    _check_chain("E8P12", k, fouts, True, True)


@pytest.mark.parametrize("with_rms,with_res", [(True, True), (False, False)])
@pytest.mark.parametrize("cbid,fouts", [("E8P12RVQ4B", (5120, 1024, 1024)), ("E8P12RVQ3B", (5120, 1024)), ("D4", (5120, 1024, 1024)),
                                        ("HI", (5120, 1024, 1024))])
def test_gemv_chain_k_plane_layouts(cbid, fouts, with_rms, with_res):
    """plain (D4), residual-scaled virtual rows (E8P12RVQ4B / RVQ3B) and the HI layout of the planes epilogue"""
    _check_chain(cbid, 5120, fouts, with_rms, with_res)


@pytest.mark.parametrize("k,fouts", [(5120, (5120, 1024)), (3584, (512,))])
def test_gemv_chain_k_row_that_is_not_finite(k, fouts):
    """an inf in the producer's GEMV output: the chain's planes carry the same not-finite marker (and the same bytes)
    as the separate launches', and the GEMV turns it into the fp path's NaN row"""
    rng = np.random.default_rng(5)
    z = rng.standard_normal((1, k)).astype(np.float16)
    z[0, k // 3] = np.inf
    h, planes = _check_chain("E8P12", k, fouts, True, True, z=_t(z))
    assert not torch.isfinite(h.float()).all()
    # the marker is in the shift word: a finite row of the same shapes has another one
    _, fin = _check_chain("E8P12", k, fouts, True, True)
    n_pad = (k + 511) // 512 * 512
    word = lambda pl: int(pl[3 * n_pad:3 * n_pad + 4].view(torch.int32)[0])   # noqa: E731
    assert all(word(a) != word(b) for a, b in zip(planes, fin))
    assert len({word(a) for a in planes}) == 1


def test_chain_k_h_against_float64_oracle():
    """module-forward bar: prev(x) finished by the chain launch is within oracle.ulp_bound (4 fp16 ulps) of the float64
    forward"""
    from quip_for_all_amd import qlinear as QL
    P = O.make_layer("E8P12", 1024, 5120, seed=21)
    prev = _layer(P)
    cons = [_layer(O.make_layer("E8P12", 5120, 512, seed=22 + i)) for i in range(2)]
    x = np.random.default_rng(3).standard_normal((1, 1024)).astype(np.float16)
    with torch.no_grad():
        z = QL.gemv_unfused(prev, torch.from_numpy(x).to(DEV))
        h, _ = QL.gemv_chain(cons, prev, z)
    What = O.qlinear_dense_weight(P)
    yref = O.qlinear_forward(P, x, "exact", What)
    err = np.abs(h.float().cpu().numpy().astype(np.float64) - yref)
    assert np.all(err <= O.ulp_bound(P, x, What)), err.max()


def _decoder_paths(dec, first):
    """tokens (eager, captured) and logits of the chain step, then of the same decoder on the plain step"""
    assert dec.chain and dec.fused_prologue
    assert not dec.qkv_fused and not dec.o_fused and not dec.attn_z        # K_left / K_right > 1: separate launches there
    assert not getattr(dec, "block_eng", False) and not dec.ffn_eng
    tc = dec.generate(10, first_token=first, use_graph=False)
    dec.reset(first)
    with torch.no_grad():
        lc = [dec.step().clone() for _ in range(3)]
    gc = dec.generate(10, first_token=first, use_graph=True)
    dec.chain = dec.fused_prologue = False
    dec.graph = None
    tp = dec.generate(10, first_token=first, use_graph=False)
    dec.reset(first)
    with torch.no_grad():
        lp = [dec.step().clone() for _ in range(3)]
    assert torch.equal(tc, tp) and torch.equal(gc, tp)
    for a, b in zip(lc, lp):
        assert torch.equal(a, b)


@pytest.mark.parametrize("hidden,ffn,heads,kv_heads,codebook", [(5120, 13824, 40, 40, "E8P12"), (3584, 18944, 28, 4, "E8P12"),
                                                                (5120, 13824, 40, 40, "D4")])
def test_decoder_with_k_factor_hidden_takes_the_chain_step(hidden, ffn, heads, kv_heads, codebook):
    """Llama-2-13B's and Qwen2-7B's block shapes: the decoder turns the chain step on by itself, and its tokens and logits
    are those of the plain three-launches-per-module step, eager and captured"""
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=hidden, ffn=ffn, layers=2, heads=heads, kv_heads=kv_heads, vocab=1024)
    dec = D.LlamaDecoder(shape, codebook, max_len=32, device=DEV, seed=5, device_init=True)
    _decoder_paths(dec, 3)


def test_from_hf_decoder_with_k_factor_hidden(monkeypatch):
    """a converted HF Llama with hidden_size 1536 = 3 x 512: from_hf turns the chain on; QUIP_CHAIN=0 keeps the old step
    and gives the same tokens"""
    transformers = pytest.importorskip("transformers")
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.quantizer import QuipQuantizer
    from tests.test_quantizer_host import _fill_random
    cfg = transformers.LlamaConfig(hidden_size=1536, intermediate_size=4096, num_hidden_layers=2, num_attention_heads=12,
                                   num_key_value_heads=4, vocab_size=320, max_position_embeddings=64,
                                   tie_word_embeddings=False)
    torch.manual_seed(4)
    model = transformers.AutoModelForCausalLM.from_config(cfg, dtype=torch.float16)
    QuipQuantizer(codebook="E8P12", inference=True, ft_epochs=0).convert_model(model)
    _fill_random(model, seed=6)
    model = model.to(DEV).eval()
    dec = LlamaDecoder.from_hf(model, max_len=64)
    assert dec.chain and dec.fused_prologue
    toks = dec.generate(12, first_token=5, use_graph=True)
    assert torch.equal(toks, dec.generate(12, first_token=5, use_graph=False))
    monkeypatch.setenv("QUIP_CHAIN", "0")
    old = LlamaDecoder.from_hf(model, max_len=64)
    assert not old.chain and not old.fused_prologue
    assert torch.equal(toks, old.generate(12, first_token=5, use_graph=True))
    assert torch.equal(toks, old.generate(12, first_token=5, use_graph=False))
