"""Batched decode without a GPU: the C ABI of the batched attention / greedy tail (declared, bound, argument checks
before any launch), the shapes of the two ops' fakes, and what LlamaDecoder.batched refuses."""
import ctypes
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("quip_rope_attn_decode_batched_f16", "quip_rope_attn_batched_workspace_bytes", "quip_argmax_step_batched_f16")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_batched_entry_points():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert set(NEW) <= names
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 9


def test_python_binding_covers_the_batched_entry_points(lib):
    from quip_for_all_amd import capi
    assert set(NEW) <= set(capi.SIGNATURES)
    for n in NEW:
        assert hasattr(lib, n)


def test_batched_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def attn(*, q=p16, batch=3, heads=4, kvh=2, hd=64, window=0):
        return lib.quip_rope_attn_decode_batched_f16(q, p16, p16, p16, p16, p16, p16, p16, p16, batch, heads, kvh, hd,
                                                     32, 0.125, window, None, None)
    assert attn(q=None) == -1                    # null pointer
    assert attn(q=p16 + 2) == -3                 # misaligned q
    assert attn(batch=0) == -2                   # batch < 1
    assert attn(heads=6, kvh=4) == -2            # heads % kv_heads
    assert attn(window=-1) == -2
    assert attn(hd=96) == -5                     # head_dim other than 64 / 128: QUIP_ERR_UNSUPPORTED
    assert lib.quip_argmax_step_batched_f16(None, 2, 8, p16, p16, None) == -1
    assert lib.quip_argmax_step_batched_f16(p16, 0, 8, p16, p16, None) == -2
    assert lib.quip_argmax_step_batched_f16(p16, 2, 0, p16, p16, None) == -2
    assert lib.quip_argmax_step_batched_f16(p16, 2, 8, p16 + 4, p16, None) == -3
    # the workspace of B sequences is B bs=1 workspaces; nonsense sizes ask for nothing
    for B in (1, 3, 16):
        assert lib.quip_rope_attn_batched_workspace_bytes(B, 32, 128) == B * lib.quip_rope_attn_workspace_bytes(32, 128)
    assert lib.quip_rope_attn_batched_workspace_bytes(0, 32, 128) == 0


def test_batched_op_fakes_on_meta_tensors():
    import quip_for_all_amd.batch_decode  # noqa: F401  (defines the two ops)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    B, H, KVH, HD, L = 3, 8, 2, 64, 40
    out = torch.ops.quip_lib.rope_attn_decode_batched(m(B, H, HD), m(B, KVH, HD), m(B, KVH, HD), m(L, HD, dtype=torch.float32),
                                                      m(L, HD, dtype=torch.float32), m(B, dtype=torch.int64),
                                                      m(B, KVH, L, HD), m(B, KVH, L, HD), None, 0)
    assert out.device.type == "meta" and tuple(out.shape) == (B, H, HD) and out.dtype == torch.float16
    assert torch.ops.quip_lib.argmax_step_batched(m(B, 100), m(B, dtype=torch.int64), m(B, dtype=torch.int64)) is None


def _stub(max_len=64, single_copy=False, head_dim=64):
    from quip_for_all_amd.decode import LlamaShape
    return types.SimpleNamespace(max_len=max_len, single_copy=single_copy, dev=torch.device("cpu"), window=0,
                                 s=LlamaShape(hidden=4 * head_dim, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512))


def test_batched_decoder_refuses_what_it_cannot_serve():
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.qlinear import QuantLinear
    for bad in (0, -1, QuantLinear.skinny_max_rows + 1):
        with pytest.raises(ValueError, match="batch"):
            LlamaDecoder.batched(_stub(), bad)
    with pytest.raises(ValueError, match="max_len"):
        LlamaDecoder.batched(_stub(max_len=64), 2, max_len=65)
    with pytest.raises(ValueError, match="single_copy"):
        LlamaDecoder.batched(_stub(single_copy=True), 2)
    with pytest.raises(NotImplementedError, match="head_dim"):
        LlamaDecoder.batched(_stub(head_dim=96), 2)
