"""The FP8 (OCP e4m3fn) KV cache without a GPU: the torch model of quantise / dequantise that the GPU tests use as their
oracle (paged_attn.quant_f8 / dequant_f8) against the format as specified -- every code, every exponent, saturation,
NaN, ties, subnormals --, the argument checks of LlamaDecoder.batched(kv_dtype=, kv_exp=), the C ABI of the two _f8
launches (declared, bound, refusals before any launch) and the ops with their fakes and operand checks."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("quip_rope_attn_decode_paged_f8", "quip_rope_attn_ragged_paged_f8")
EXPS = range(-8, 8)


def _codes():
    """the 254 non-NaN bytes"""
    return torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8)


def _value(c):
    """e4m3fn by its definition: 1 sign, 4 exponent bits (bias 7), 3 mantissa bits, subnormals, no infinities"""
    s, e, m = c >> 7, (c >> 3) & 15, c & 7
    v = m * 2.0 ** -9 if e == 0 else (1 + m / 8.0) * 2.0 ** (e - 7)
    return -v if s else v


def test_every_code_is_an_exact_finite_fp16_value_and_survives_the_round_trip():
    from quip_for_all_amd.paged_attn import dequant_f8, quant_f8
    codes = _codes()
    assert codes.numel() == 254
    for e in EXPS:
        x = dequant_f8(codes, e)
        assert x.dtype == torch.float16 and bool(torch.isfinite(x).all())
        want = torch.tensor([_value(int(c)) * 2.0 ** e for c in codes], dtype=torch.float64)
        assert torch.equal(x.double(), want), e                         # exact: no bit lost in fp16
        assert torch.equal(quant_f8(x, e), codes), e                    # (-0 -> 0x80 included)


def test_the_exact_range_of_exponents_is_wider_than_the_one_allowed():
    codes = _codes()
    vals = torch.tensor([_value(int(c)) for c in codes], dtype=torch.float64)
    for e in range(-15, 8):
        y = (vals * 2.0 ** e).to(torch.float16)
        assert bool(torch.isfinite(y).all()) and torch.equal(y.double(), vals * 2.0 ** e), e
    assert not bool(torch.isfinite((vals * 2.0 ** 8).to(torch.float16)).all())                  # 448 * 256 overflows
    assert not torch.equal((vals * 2.0 ** -16).to(torch.float16).double(), vals * 2.0 ** -16)   # subnormal bits drop


def test_saturation_nan_ties_and_subnormals():
    from quip_for_all_amd.paged_attn import dequant_f8, quant_f8
    inf, nan = float("inf"), float("nan")
    for e in (0, -8, -3, 2, 7):
        s = 2.0 ** e
        q = lambda *v: quant_f8(torch.tensor(v, dtype=torch.float32) * s, e).tolist()  # noqa: E731
        assert q(448.0, 449.0, 464.0, 1e4, inf) == [0x7e] * 5
        assert q(-448.0, -465.0, -1e4, -inf) == [0xfe] * 4
        assert all(b & 0x7f == 0x7f for b in q(nan, -nan))
        # ties go to the even mantissa: 17 between 16 (0x58) and 18 (0x59), 19 between 18 and 20 (0x5a); 416 + 16 = 432
        # between 416 (0x7d) and 448 (0x7e)
        assert q(17.0, 19.0, 432.0, -17.0) == [0x58, 0x5a, 0x7e, 0xd8]
        # subnormals (steps of 2^-9): half the smallest ties to zero, just above it rounds up, 1.5 steps ties to 2 steps,
        # 2.5 steps to 2 steps; the smallest normal is 2^-6 = 0x08
        u = 2.0 ** -9
        assert q(0.5 * u, 0.5 * u * 1.001, 1.5 * u, 2.5 * u, -0.5 * u, 7.5 * u, 2.0 ** -6) == [0, 1, 2, 2, 0x80, 8, 8]
    # fp16 inputs go through fp32 unchanged
    x = torch.tensor([0.3, -7.7, 300.0, 6e4], dtype=torch.float16)
    assert torch.equal(quant_f8(x, -3), quant_f8(x.float(), -3))
    # at e = 2: 0.075 -> 0.078125 (a subnormal step is 2^-9), -1.925 -> -1.875, 75 -> 72, 15000 -> 448
    assert dequant_f8(quant_f8(x, 2), 2).tolist() == [0.3125, -7.5, 288.0, 1792.0]


def test_batched_refuses_fp8_without_paged_and_bad_exponents():
    from quip_for_all_amd.decode import LlamaDecoder
    from quip_for_all_amd.paged_cache import PagedBatchDecoder
    with pytest.raises(ValueError, match="paged"):
        LlamaDecoder.batched(object(), 2, kv_dtype="fp8")
    with pytest.raises(ValueError, match="paged"):
        LlamaDecoder.batched(object(), 2, kv_exp=[[0, 0]])

    class Parent:
        class s:
            layers = 3
    with pytest.raises(ValueError, match="kv_dtype"):
        PagedBatchDecoder(Parent, 2, 64, kv_dtype="fp4")
    with pytest.raises(ValueError, match="kv_exp"):
        PagedBatchDecoder(Parent, 2, 64, kv_dtype="fp16", kv_exp=[[0, 0]] * 3)
    check = PagedBatchDecoder._check_kv_exp
    assert check(None, 3) == [[0, 0]] * 3
    assert check([[-8, 7], [0, 1], (2, -3)], 3) == [[-8, 7], [0, 1], [2, -3]]
    assert check(torch.tensor([[-8, 7], [0, 1], [2, -3]]), 3) == [[-8, 7], [0, 1], [2, -3]]
    for bad in ([[0, 0]] * 2, [[0, 0, 0]] * 3, [0, 0, 0], 5, [[0, 8]] * 3, [[-9, 0]] * 3, [[0.0, 0]] * 3, [[True, 0]] * 3,
                torch.zeros(3, 2), torch.zeros(2, 3, dtype=torch.int64)):
        with pytest.raises(ValueError, match="kv_exp"):
            check(bad, 3)
        with pytest.raises(ValueError, match="kv_exp"):
            PagedBatchDecoder(Parent, 2, 64, kv_dtype="fp8", kv_exp=bad)


# ---- the C ABI and the ops
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_both_entries_and_the_abi_version_moved():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert set(ENTRIES) <= declared
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 16


def test_python_binding_covers_both_entries(lib):
    from quip_for_all_amd import capi
    f16 = ("quip_rope_attn_decode_paged_f16", "quip_rope_attn_ragged_paged_f16")
    for new, old in zip(ENTRIES, f16):                                   # the _f16 signature plus two ints
        assert capi.SIGNATURES[new] == capi.SIGNATURES[old] + [ctypes.c_int32] * 2
    assert all(hasattr(lib, e) for e in ENTRIES)
    assert lib.quip_abi_version() >= 16
    assert set(ENTRIES) <= set(capi.check_symbols())


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def dec(*, q=p16, pos=p16, table=p16, kpool=p16, batch=3, heads=4, kvh=2, hd=64, max_len=384, n_pages=20, max_pages=6,
            window=0, ws=None, k_exp=0, v_exp=0):
        return lib.quip_rope_attn_decode_paged_f8(q, p16, p16, p16, p16, pos, table, kpool, p16, p16, batch, heads, kvh, hd,
                                                  max_len, n_pages, max_pages, 0.125, window, ws, None, k_exp, v_exp)

    def rag(*, q=p16, out=p16, pos=p16, table=p16, slots=(2, 0), seg_rows=(5, 70), rows=None, heads=4, kvh=2, hd=64,
            max_len=384, batch=3, n_pages=20, max_pages=6, window=0, k_exp=0, v_exp=0):
        n = len(slots)
        sl, sr = (ctypes.c_int32 * n)(*slots), (ctypes.c_int32 * n)(*seg_rows)
        return lib.quip_rope_attn_ragged_paged_f8(q, p16, p16, p16, p16, pos, table, p16, p16, out,
                                                  sum(seg_rows) if rows is None else rows, heads, kvh, hd, max_len, batch,
                                                  n_pages, max_pages, ctypes.addressof(sl), ctypes.addressof(sr), n, 0.125,
                                                  window, None, k_exp, v_exp)
    for f in (dec, rag):
        for e in (-9, 8, 100, -128):                                                              # QUIP_ERR_BAD_SHAPE
            assert f(k_exp=e) == -2 and f(v_exp=e) == -2
        # everything the _f16 entries refuse
        assert f(q=None) == -1 and f(table=None) == -1 and f(pos=None) == -1                      # QUIP_ERR_NULL_POINTER
        assert f(n_pages=0) == -2 and f(max_pages=0) == -2 and f(max_len=0) == -2
        assert f(max_len=385) == -2
        assert f(heads=6, kvh=4) == -2 and f(window=-1) == -2 and f(batch=0) == -2
        assert f(hd=96) == -5                                                                     # QUIP_ERR_UNSUPPORTED
        assert f(q=p16 + 2) == -3 and f(table=p16 + 2) == -3 and f(pos=p16 + 4) == -3             # QUIP_ERR_MISALIGNED
    assert dec(kpool=None) == -1 and dec(ws=p16 + 4) == -3
    assert dec(max_pages=8193, max_len=64) == -5
    assert rag(slots=(2, 2)) == -2 and rag(slots=(2, 3)) == -2 and rag(rows=76) == -2 and rag(seg_rows=(5, 0)) == -2


def _meta(*s, dtype=torch.float16):
    return torch.empty(*s, dtype=dtype, device="meta")


def test_ops_and_fakes_are_registered():
    import quip_for_all_amd.paged_attn  # noqa: F401  (defines the ops)
    m = _meta
    R, H, KVH, HD, L, B, NP, MP = 7, 8, 2, 64, 100, 3, 9, 2
    f32, u8, tab = torch.float32, torch.uint8, m(B, MP, dtype=torch.int32)
    out = torch.ops.quip_lib.rope_attn_ragged_paged_f8(m(R, H, HD), m(R, KVH, HD), m(R, KVH, HD), m(L, HD, dtype=f32),
                                                       m(L, HD, dtype=f32), m(B, dtype=torch.int64), [2, 0], [4, 3], tab,
                                                       m(NP, KVH, 64, HD, dtype=u8), m(NP, KVH, 64, HD, dtype=u8), 16, -3, 2)
    assert out.device.type == "meta" and tuple(out.shape) == (R, H, HD) and out.dtype == torch.float16
    out = torch.ops.quip_lib.rope_attn_decode_paged_f8(m(B, H, HD), m(B, KVH, HD), m(B, KVH, HD), m(L, HD, dtype=f32),
                                                       m(L, HD, dtype=f32), m(B, dtype=torch.int64), tab,
                                                       m(NP, KVH, 64, HD, dtype=u8), m(NP, KVH, 64, HD, dtype=u8), None, 0,
                                                       -8, -8)
    assert out.device.type == "meta" and tuple(out.shape) == (B, H, HD) and out.dtype == torch.float16


def test_wrappers_refuse_pools_of_the_other_dtype_and_bad_exponents():
    """the operand checks run before anything touches a device: CPU tensors get as far as the pool dtype"""
    from quip_for_all_amd import paged_attn as P
    R, H, KVH, HD, L, B, NP, MP = 3, 4, 2, 64, 128, 3, 5, 2
    t = lambda *s, dtype=torch.float16: torch.zeros(*s, dtype=dtype)  # noqa: E731
    q, k, v = t(R, H, HD), t(R, KVH, HD), t(R, KVH, HD)
    cos, sin, pos = t(L, HD, dtype=torch.float32), t(L, HD, dtype=torch.float32), t(B, dtype=torch.int64)
    tab = t(B, MP, dtype=torch.int32)
    p16, p8 = t(NP, KVH, 64, HD), t(NP, KVH, 64, HD, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        P._rope_attn_decode_paged_f8_cuda(q, k, v, cos, sin, pos, tab, p16, p16.clone())
    with pytest.raises(ValueError, match="uint8"):
        P._rope_attn_decode_paged_f8_cuda(q, k, v, cos, sin, pos, tab, p8, p16)
    with pytest.raises(ValueError, match="uint8"):
        P._rope_attn_ragged_paged_f8_cuda(q, k, v, cos, sin, pos, [0], [3], tab, p16, p16.clone())
    with pytest.raises(ValueError, match="uint8"):
        P._rope_attn_ragged_paged_f8_cuda(q, k, v, cos, sin, pos, [0], [3], tab, p8, p8.view(torch.float8_e4m3fn))
    with pytest.raises(ValueError, match="fp16"):
        P._rope_attn_decode_paged_cuda(q, k, v, cos, sin, pos, tab, p8, p8.clone())
    with pytest.raises(ValueError, match="fp16"):
        P._rope_attn_ragged_paged_cuda(q, k, v, cos, sin, pos, [0], [3], tab, p16, p8)
    for ke, ve in ((-9, 0), (0, 8)):
        with pytest.raises(ValueError, match="exponents"):
            P._check_exps("op", ke, ve)
    assert P._check_exps("op", -8, 7) == (-8, 7)
