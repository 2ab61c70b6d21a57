"""The whole-token launch without a GPU: quip_block_engine_token is declared, bound and checks its arguments before any
launch; the op's fake; the op lives outside register_lib._SCHEMAS; what the launch's hop counter can take."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_entry_and_the_abi_version_moved():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert "quip_block_engine_token" in set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert "quip_token_tail_args" in src
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 10


def test_python_binding_and_struct_mirror(lib):
    from quip_for_all_amd import capi
    assert capi.SIGNATURES["quip_block_engine_token"] == [ctypes.c_void_p] * 3
    assert hasattr(lib, "quip_block_engine_token")
    # seven pointers and an int32, padded to the pointer size: the C struct's layout
    assert [f[0] for f in capi.TokenTailArgs._fields_] == ["tok", "pos", "embed", "final_norm", "lm_head", "logits", "xnorm", "vocab"]
    assert ctypes.sizeof(capi.TokenTailArgs) == 64
    # quip_block_engine and its struct did not change
    assert capi.SIGNATURES["quip_block_engine"] == [ctypes.c_void_p] * 2
    assert ctypes.sizeof(capi.BlockEngineArgs) == 112


def test_argument_validation_without_gpu(lib):
    from quip_for_all_amd import capi
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 63) & ~63

    def call(*, layers=a, pos=a, tpos=None, ws=a, grid=a, h_out=None, tok=a, embed=a, norm=a, lm=a, logits=a, xnorm=None,
             vocab=32000, n_layers=2, max_len=16, shape=0, codebook=0, grid2=None, no_tail=False, no_args=False):
        A = capi.BlockEngineArgs(layers, None, h_out, pos, a, a, grid, ws, None, n_layers, max_len, -1, 1e-5, 0.1, codebook, 0.0,
                                 shape, grid2)
        T = capi.TokenTailArgs(tok, pos if tpos is None else tpos, embed, norm, lm, logits, xnorm, vocab)
        return lib.quip_block_engine_token(None if no_args else ctypes.byref(A), None if no_tail else ctypes.byref(T), None)

    assert call(no_args=True) == -1 and call(no_tail=True) == -1
    for k in ("layers", "pos", "ws", "grid", "tok", "embed", "norm", "lm", "logits"):
        assert call(**{k: None}) == -1, k                       # QUIP_ERR_NULL_POINTER
    for k in ("layers", "ws", "embed", "norm", "lm", "logits", "h_out", "xnorm"):
        assert call(**{k: a + 2}) == -3, k                      # 16-byte alignment
    assert call(grid=a + 16) == -3                              # the table: 64 bytes
    assert call(tok=a + 4) == -3 and call(pos=a + 4, tpos=a + 4) == -3      # int64 scalars
    assert call(vocab=255) == -2 and call(vocab=0) == -2 and call(vocab=256 * 65535) == -2
    assert call(n_layers=0) == -2 and call(max_len=0) == -2
    assert call(tpos=a + 8) == -2                               # the tail advances the counter the blocks read
    assert call(shape=1) == -5 and call(shape=3) == -5          # QUIP_ERR_UNSUPPORTED: the 8192-wide launch has no tail
    assert call(codebook=4) == -1 and call(codebook=4, grid2=a + 4) == -3
    assert call(n_layers=147) == -2                             # 7 hand-offs per block + the tail's: a 10-bit counter


def test_hop_counter_holds_the_tail():
    """the launchers admit n_layers <= 146: 7 hand-offs per block + 1 for the arg-max = 1023, the counter's last value"""
    src = open(os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_block.hip")).read()
    limits = [int(x) for x in re.findall(r"in\.n_layers > (\d+)\) return QUIP_ERR_BAD_SHAPE", src)]
    assert limits and all(7 * n + 1 <= 1023 for n in limits), limits
    assert "<< 10" in re.search(r"const uint32_t ebase = .*", src).group(0)


def test_op_is_defined_outside_the_pinned_schemas_and_has_a_fake():
    import quip_for_all_amd.token_tail  # noqa: F401  (defines the op)
    from quip_for_all_amd import register_lib as R
    assert "block_engine_token" not in R._SCHEMAS
    assert hasattr(torch.ops.quip_lib, "block_engine_token")
    schema = str(torch.ops.quip_lib.block_engine_token.default._schema)
    for mutated in ("Tensor(a!) tok", "Tensor(b!) pos", "Tensor(c!) logits", "Tensor(d!) workspace"):
        assert mutated in schema, schema
    assert schema.endswith("-> ()")
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    U8, I64, F32 = torch.uint8, torch.int64, torch.float32
    out = torch.ops.quip_lib.block_engine_token(m(512, dtype=U8), m(1, dtype=I64), m(1, dtype=I64), m(32000, 4096), m(4096),
                                                m(32000, 4096), m(1, 32000), m(8, 128, dtype=F32), m(8, 128, dtype=F32),
                                                m(256, dtype=I64), m(1 << 20, dtype=U8), 2, 8, 1e-5, 0.088)
    assert out is None


def test_step_keeps_the_separate_tail_where_the_launch_cannot_serve():
    """sampling, the 8192-wide launch, a switched-off engine and QUIP_TOKEN_TAIL=0 stay on _head"""
    import types
    from quip_for_all_amd.decode import LlamaDecoder
    t = lambda *shape, cuda=True: types.SimpleNamespace(is_cuda=cuda, dtype=torch.float16, is_contiguous=lambda: True,  # noqa: E731
                                                        dim=lambda: len(shape), shape=torch.Size(shape), device="gpu")
    lm = t(512, 4096)

    def stub(**kw):
        d = dict(block_eng=True, token_tail=True, sampling=None, eng_shape=0, lm_head=lm, embed=lm,
                 final_norm=t(4096), layers=[None] * 32)
        d.update(kw)
        return types.SimpleNamespace(**d)
    on = LlamaDecoder._token_tail_on
    assert on(stub()) and on(stub(eng_shape=2))
    for kw in (dict(block_eng=False), dict(token_tail=False), dict(sampling=(0.7, None)), dict(eng_shape=1),
               dict(lm_head=t(512, 4096, cuda=False)), dict(lm_head=t(255, 4096), embed=t(255, 4096)), dict(embed=t(500, 4096)),
               dict(layers=[None] * 147)):
        assert not on(stub(**kw)), kw
