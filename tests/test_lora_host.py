"""LoRA adapters without a GPU: the C ABI of the two launches (declared, bound, shape errors before any launch), the ops'
fakes, PEFT directories read back (safetensors and .bin), what a config is refused for, the adapter registry on a stub
model, and the float64 reference helpers the GPU tests rely on."""
import ctypes
import json
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("quip_lora_shrink_rows_f16", "quip_lora_expand_rows_f16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_both_entries_and_the_abi_version(lib):
    hdr = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(NEW) <= set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    assert abi >= 20
    assert lib.quip_abi_version() == abi
    from quip_for_all_amd import capi
    assert set(NEW) <= set(capi.SIGNATURES)
    for n in NEW:
        assert hasattr(lib, n)


def test_argument_validation_without_gpu(lib):
    """null / misaligned pointers and every shape rule answer their code before anything is launched"""
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def shrink(*, x=p16, A=p16, idx=p16, t=p16, rows=2, n_in=64, R=16, n=3, mode=0, aux=None):
        return lib.quip_lora_shrink_rows_f16(x, A, idx, t, rows, n_in, R, n, mode, aux, 1e-5, None)
    assert shrink(x=None) == -1 and shrink(A=None) == -1 and shrink(idx=None) == -1 and shrink(t=None) == -1
    assert shrink(mode=1) == -1 and shrink(mode=2) == -1            # (the norm weight / the gate is missing)
    assert shrink(x=p16 + 2) == -3 and shrink(A=p16 + 8) == -3 and shrink(idx=p16 + 2) == -3 and shrink(t=p16 + 2) == -3
    assert shrink(mode=1, aux=p16 + 2) == -3
    assert shrink(rows=0) == -2 and shrink(n=0) == -2 and shrink(mode=3, aux=p16) == -2
    assert shrink(n_in=0) == -2 and shrink(n_in=4) == -2 and shrink(n_in=68) == -2
    assert shrink(R=0) == -2 and shrink(R=12) == -2
    assert shrink(n_in=28680) == -5 and shrink(R=200) == -5

    P3, I3 = ctypes.c_void_p * 3, ctypes.c_int32 * 3

    def expand(*, t=p16, idx=p16, scale=p16, rows=2, Rt=24, n=3, nseg=2, y=(p16, p16, None), B=(p16, p16, None),
               out=(64, 8, 0), R=(8, 16, 8), r0=(0, 8, 0)):
        return lib.quip_lora_expand_rows_f16(t, idx, scale, rows, Rt, n, nseg, P3(*y), P3(*B), I3(*out), I3(*R), I3(*r0), None)
    assert expand(t=None) == -1 and expand(idx=None) == -1 and expand(scale=None) == -1
    assert expand(y=(None, p16, None)) == -1 and expand(B=(p16, None, None)) == -1
    assert expand(t=p16 + 2) == -3 and expand(B=(p16 + 8, p16, None)) == -3 and expand(y=(p16 + 1, p16, None)) == -3
    assert expand(rows=0) == -2 and expand(nseg=0) == -2 and expand(nseg=4) == -2 and expand(n=0) == -2
    assert expand(Rt=12) == -2 and expand(Rt=0) == -2 and expand(Rt=200) == -5
    assert expand(out=(60, 8, 0)) == -2 and expand(out=(-8, 8, 0)) == -2
    assert expand(R=(12, 16, 8)) == -2 and expand(R=(0, 16, 8)) == -2
    assert expand(r0=(4, 8, 0)) == -2 and expand(r0=(0, 16, 0)) == -2          # (ranks [16, 32) of 24)
    # every segment skipped (out_j = 0, pointers not looked at): nothing to launch, no error
    assert expand(y=(None, None, None), B=(None, None, None), out=(0, 0, 0)) == 0


def test_op_fakes_on_meta_tensors():
    import quip_for_all_amd.lora  # noqa: F401  (defines the two ops)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    i32, f32 = torch.int32, torch.float32
    for kw in ({}, {"rms_weight": m(688), "rms_eps": 1e-5}, {"gate": m(5, 688)}):
        t = torch.ops.quip_lib.lora_shrink_rows(m(5, 688), m(4, 48, 688), m(5, dtype=i32), **kw)
        assert t.device.type == "meta" and tuple(t.shape) == (5, 48) and t.dtype == f32
    ys = [m(5, 256), m(5, 0), m(5, 128)]
    assert torch.ops.quip_lib.lora_expand_rows(m(5, 48, dtype=f32), ys, [m(4, 256, 16), m(4, 0, 16), m(4, 128, 16)],
                                               m(4, 3, dtype=f32), m(5, dtype=i32), [0, 16, 32]) is None


# ---- PEFT's files and configs -------------------------------------------------------------------------------------------------
DIMS = {"q": (32, 32), "k": (32, 16), "v": (32, 16), "o": (32, 32), "gate": (32, 48), "up": (32, 48), "down": (48, 32)}
PEFT = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
        "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}


def make_adapter(dims, n_layers, r, targets, seed, amp=1.0, prefix="base_model.model.model."):
    """random adapter tensors in PEFT's key scheme"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(n_layers):
        for mod in targets:
            n_in, n_out = dims[mod]
            out[f"{prefix}layers.{i}.{PEFT[mod]}.lora_A.weight"] = \
                (amp * torch.randn(r, n_in, generator=g) / n_in ** 0.5).to(torch.float16)
            out[f"{prefix}layers.{i}.{PEFT[mod]}.lora_B.weight"] = (amp * torch.randn(n_out, r, generator=g)).to(torch.float16)
    return out


def config(r, targets, **kw):
    c = {"peft_type": "LORA", "r": r, "lora_alpha": 2 * r, "target_modules": [PEFT[t].split(".")[1] for t in targets],
         "bias": "none", "use_rslora": False, "use_dora": False, "modules_to_save": None, "rank_pattern": {},
         "alpha_pattern": {}, "fan_in_fan_out": False}
    c.update(kw)
    return c


@pytest.mark.parametrize("fmt", ["safetensors", "bin"])
def test_read_peft_dir_round_trip(tmp_path, fmt):
    from quip_for_all_amd.lora import read_peft_dir
    tensors, cfg = make_adapter(DIMS, 2, 4, ("q", "v"), seed=1), config(4, ("q", "v"))
    with open(tmp_path / "adapter_config.json", "w") as f:
        json.dump(cfg, f)
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(tensors, str(tmp_path / "adapter_model.safetensors"))
    else:
        torch.save(tensors, tmp_path / "adapter_model.bin")
    got, got_cfg = read_peft_dir(str(tmp_path))
    assert got_cfg == cfg and set(got) == set(tensors)
    for k in tensors:
        assert torch.equal(got[k], tensors[k])
    with pytest.raises(FileNotFoundError):
        os.remove(tmp_path / ("adapter_model." + fmt))
        read_peft_dir(str(tmp_path))


def test_check_config_serves_and_refuses_by_field():
    from quip_for_all_amd.lora import check_config
    r, scale, targets = check_config(config(4, ("v", "q")), 16)
    assert (r, scale, targets) == (4, 2.0, ["q", "v"])
    assert check_config(config(4, ("o", "down"), use_rslora=True, lora_alpha=6), 16)[1] == 3.0           # alpha / sqrt(r)
    assert check_config(config(8, tuple(DIMS)), 8)[2] == list(DIMS)
    for field, kw in (("use_dora", {"use_dora": True}), ("bias", {"bias": "all"}), ("bias", {"bias": "lora_only"}),
                      ("modules_to_save", {"modules_to_save": ["lm_head"]}), ("rank_pattern", {"rank_pattern": {"q_proj": 8}}),
                      ("alpha_pattern", {"alpha_pattern": {"q_proj": 8}}), ("fan_in_fan_out", {"fan_in_fan_out": True}),
                      ("target_modules", {"target_modules": ["q_proj", "lm_head"]}), ("target_modules", {"target_modules": []}),
                      ("target_modules", {"target_modules": "all-linear"}), ("r", {"r": 32}), ("r", {"r": 0}),
                      ("peft_type", {"peft_type": "IA3"})):
        with pytest.raises(NotImplementedError, match=field):
            check_config({**config(4, ("q",)), **kw}, 16)


def _stub_decoder(n_layers=2):
    mod = lambda d: types.SimpleNamespace(in_features=d[0], out_features=d[1])  # noqa: E731
    return types.SimpleNamespace(dev=torch.device("cpu"), layers=[{m: mod(d) for m, d in DIMS.items()} for _ in range(n_layers)])


def test_registry_load_unload_reload_and_shape_refusals():
    from quip_for_all_amd.lora import LoraState
    st = LoraState(_stub_decoder(), max_adapters=2, max_rank=12)
    assert st.rank == 16 and st.index(None) == -1 and not st.active("q")
    changed = []
    st.on_launches_changed = lambda: changed.append(1)
    a = make_adapter(DIMS, 2, 4, ("q", "v"), seed=1)
    assert st.load("a", a, config(4, ("q", "v"))) == 0 and st.index("a") == 0 and len(changed) == 1
    assert st.active("q") and st.active("v") and not st.active("k")
    A = st.layers[1].A["qkv"]
    assert tuple(A.shape) == (2, 48, 32) and tuple(st.layers[1].B["v"].shape) == (2, 16, 16)
    assert torch.equal(A[0, 0:4], a["base_model.model.model.layers.1.self_attn.q_proj.lora_A.weight"])
    assert torch.equal(A[0, 32:36], a["base_model.model.model.layers.1.self_attn.v_proj.lora_A.weight"])
    assert not A[0, 4:32].any() and not A[0, 36:].any() and not A[1].any()          # padding and k's ranks stay zero
    assert torch.equal(st.layers[1].B["v"][0, :, :4], a["base_model.model.model.layers.1.self_attn.v_proj.lora_B.weight"])
    assert st.scale[0].tolist() == [2.0, 2.0, 2.0] and st.scale[1].tolist() == [0.0, 0.0, 0.0]
    ptr = A.data_ptr()
    b = make_adapter(DIMS, 2, 12, tuple(DIMS), seed=2)
    assert st.load("b", b, config(12, tuple(DIMS), use_rslora=True)) == 1 and len(changed) == 2
    with pytest.raises(RuntimeError, match="max_adapters"):
        st.load("c", a, config(4, ("q", "v")))
    # reload under a name: same slot, the old entries gone (q, v of rank 4 -> o of rank 2)
    o = make_adapter(DIMS, 2, 2, ("o",), seed=3)
    assert st.load("a", o, config(2, ("o",))) == 0 and len(changed) == 2            # (the launching groups did not change)
    assert not st.layers[1].A["qkv"][0].any() and st.layers[0].A["o"][0, :2].any() and st.layers[1].A["qkv"][1].any()
    st.unload("b")
    assert st.names == ["a", None] and not st.layers[0].A["gu"].any() and not st.scale[1].any() and len(changed) == 3
    assert st.active("o") and not st.active("q")
    with pytest.raises(KeyError):
        st.index("b")
    assert st.load("c", a, config(4, ("q", "v"))) == 1
    assert st.layers[1].A["qkv"].data_ptr() == ptr                                  # fixed addresses
    # tensors that do not match the model or the config: refused before anything is written
    snap = st.layers[0].A["qkv"].clone()
    wrong = dict(a)
    key = "base_model.model.model.layers.0.self_attn.q_proj.lora_A.weight"
    wrong[key] = torch.zeros(4, 40, dtype=torch.float16)
    with pytest.raises(ValueError, match="shape"):
        st.load("c", wrong, config(4, ("q", "v")))
    missing = {k: v for k, v in a.items() if k != key}
    with pytest.raises(ValueError, match="missing"):
        st.load("c", missing, config(4, ("q", "v")))
    with pytest.raises(ValueError, match="target_modules"):
        st.load("c", a, config(4, ("q",)))
    with pytest.raises(ValueError, match="layers"):
        st.load("c", make_adapter(DIMS, 3, 4, ("q", "v"), seed=1), config(4, ("q", "v")))
    with pytest.raises(ValueError, match="not a lora_A"):
        st.load("c", {**a, "base_model.model.lm_head.lora_A.weight": torch.zeros(4, 32)}, config(4, ("q", "v")))
    with pytest.raises(NotImplementedError, match="max_rank"):
        st.load("c", make_adapter(DIMS, 2, 13, ("q",), seed=1), config(13, ("q",)))
    assert torch.equal(st.layers[0].A["qkv"], snap)
    assert st.bytes_per_slot() == 2 * 2 * (16 * (3 * 32 + 32 + 2 * 32 + 48) + 16 * (32 + 16 + 16 + 32 + 48 + 48 + 32))


def test_float64_reference_helpers():
    """shrink_ref / expand_ref on a case small enough to state by hand, and the three input modes against torch"""
    from quip_for_all_amd.lora import expand_ref, shrink_ref, xin_ref
    x = torch.tensor([[1.0, -2.0, 0.5, 4.0], [2.0, 2.0, 2.0, 2.0]], dtype=torch.float16)
    A = torch.tensor([[[1.0, 1.0, 1.0, 1.0], [1.0, -1.0, 0.0, 2.0]], [[0.5, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, -1.0]]],
                     dtype=torch.float16)
    idx = torch.tensor([1, -1], dtype=torch.int32)
    t, mag, gmag = shrink_ref(x, A, idx)
    assert t.tolist() == [[0.5, -4.0], [0.0, 0.0]] and mag.tolist() == [[0.5, 4.0], [0.0, 0.0]] and not gmag.any()
    t0, mag0, _ = shrink_ref(x, A, torch.tensor([0, 0], dtype=torch.int32))
    assert t0.tolist() == [[3.5, 11.0], [8.0, 4.0]] and mag0.tolist() == [[7.5, 11.0], [8.0, 8.0]]
    w = torch.tensor([1.0, 0.5, 2.0, 1.0], dtype=torch.float16)
    want = torch.nn.functional.rms_norm(x.double(), (4,), w.double(), float(np.float32(1e-5))).numpy()
    np.testing.assert_allclose(xin_ref(x, rms_weight=w, rms_eps=1e-5), want, rtol=1e-14)
    g = torch.tensor([[0.0, 1.0, -1.0, 8.0], [-8.0, 2.0, 0.5, 0.25]], dtype=torch.float16)
    np.testing.assert_allclose(xin_ref(x, gate=g), (x.double() * torch.nn.functional.silu(g.double())).numpy(), rtol=1e-14)
    _, magg, gmagg = shrink_ref(x, A, idx, gate=g)
    prod = np.abs(A[1].double().numpy() * xin_ref(x, gate=g)[0][None])
    np.testing.assert_allclose(magg[0], prod.sum(-1))
    np.testing.assert_allclose(gmagg[0], (prod * (np.abs(g[0].double().numpy()) + 6.0)[None]).sum(-1))
    # expand: y (2, 2), B (2 adapters, 2 outputs, 2 ranks) read from ranks [2, 4) of t
    y = torch.tensor([[1.0, -1.0], [3.0, 4.0]], dtype=torch.float16)
    B = torch.tensor([[[1.0, 0.0], [0.0, 1.0]], [[2.0, 1.0], [-1.0, 0.5]]], dtype=torch.float16)
    tt = torch.tensor([[9.0, 9.0, 1.0, 2.0], [9.0, 9.0, 5.0, 6.0]], dtype=torch.float32)
    scale = torch.tensor([[1.0, 1.0, 1.0], [0.0, 0.5, 0.0]], dtype=torch.float32)
    out, m = expand_ref(y, B, tt, scale, idx, 1, 2)
    assert out.tolist() == [[1.0 + 0.5 * 4.0, -1.0 + 0.5 * 0.0], [3.0, 4.0]]
    assert m.tolist() == [[1.0 + 0.5 * 4.0, 1.0 + 0.5 * 2.0], [3.0, 4.0]]


def test_decoder_side_without_a_gpu():
    """enable_lora on a CPU-built decoder: the switches, the state through a re-run of the runtime set-up, the index tensors of
    the bs = 1 decoder and of the slots (fork copies, free clears, reset keeps), captured steps dropped when the launching
    groups change"""
    from quip_for_all_amd import decode as D
    np.random.seed(11)
    dec = D.LlamaDecoder(D.TINY, "E8P12", max_len=128, device="cpu", seed=3)
    with pytest.raises(RuntimeError, match="enable_lora"):
        dec.set_adapter(None)
    bd0 = dec.batched(2)                      # (made before enable_lora: it serves adapters all the same)
    dec.enable_lora(max_adapters=2, max_rank=12)
    assert dec.lora.rank == 16 and not dec.block_eng and not dec.ffn_eng and not dec.attn_z and not dec._token_tail_on()
    assert dec.lora.idx.dtype == torch.int32 and dec.lora.idx.tolist() == [-1] and dec.lora_fused_step
    s = D.TINY
    dims = {"q": (s.hidden, s.q_width), "k": (s.hidden, 128), "v": (s.hidden, 128), "o": (s.q_width, s.hidden),
            "gate": (s.hidden, s.ffn), "up": (s.hidden, s.ffn), "down": (s.ffn, s.hidden)}
    bd0.graph = dec.graph = "captured"
    assert dec.load_adapter("a", make_adapter(dims, 2, 4, ("q", "v"), seed=1), config(4, ("q", "v"))) == 0
    assert dec.graph is None and bd0.graph is None          # q / k / v's launches joined the step
    bd0.graph = dec.graph = "captured"
    assert dec.load_adapter("b", make_adapter(dims, 2, 8, ("v",), seed=2), config(8, ("v",))) == 1
    assert dec.graph == "captured" and bd0.graph == "captured"
    dec.set_adapter("b")
    assert dec.lora.idx.tolist() == [1]
    ptr = dec.lora.idx.data_ptr()
    dec._init_runtime()
    assert dec.lora.idx.data_ptr() == ptr and dec.lora.idx.tolist() == [1] and dec.layers[1]["lora"] is dec.lora.layers[1]
    assert not dec.ffn_eng and not dec.attn_z and not dec.block_eng
    assert dec._rows_adapter(None, 1) is dec.lora.idx and dec._rows_adapter(None, 3).tolist() == [1, 1, 1]
    for bd in (bd0, dec.batched(3, paged=True)):
        assert bd.slot_adapter.dtype == torch.int32 and set(bd.slot_adapter.tolist()) == {-1}
        bd.set_slot_adapter(1, "a")
        bd.set_slot_adapter(0, "b")
        bd.reset()
        assert bd.slot_adapter.tolist()[:2] == [1, 0]
        with pytest.raises(KeyError):
            bd.set_slot_adapter(0, "c")
    bd.fork_slot(0, 2)
    assert bd.slot_adapter.tolist() == [1, 0, 1]
    bd.free_slot(0)
    assert bd.slot_adapter.tolist() == [-1, 0, 1]
    bd.graph = "captured"
    dec.unload_adapter("a")                   # q leaves the launching groups
    assert bd.graph is None and dec.lora.names == [None, "b"]
