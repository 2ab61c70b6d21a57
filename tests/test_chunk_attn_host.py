"""The chunked prompt pass without a GPU: the C ABI of the chunk attention launch (declared, bound, argument checks before
any launch), the op's fake, what extend / extend_slot refuse, and a CPU model of the launch's arithmetic
(csrc/chunk_attn.hip.h) whose distance from float64 attention sets the bound the GPU test holds the kernel to.

Error unit: u = 2^-11 * max|v| over the keys a row attends to.  The bound is 1.5 u: 0.5 u from rounding the output to
fp16 (|out| <= max|v|, half an fp16 ulp of a value below max|v|), 0.5 u from rounding the probabilities to fp16 before
the product with V (relative error 2^-11 on every p, the weights sum to one), and the fp32 terms (scores over 128
products, the running sum over <= 512 keys, the accumulation) stay below 0.05 u at these lengths."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "quip_rope_attn_chunk_f16"
BOUND_U = 1.5
TILE = 64

# the shapes of tests/test_gpu_chunk_attn.py
SHAPES = ((4, 2, 64), (8, 2, 128), (4, 4, 128))            # heads, kv_heads, head_dim
CHUNKS = ((1, 0), (5, 3), (33, 61), (70, 130), (64, 300))   # rows, pos
WINDOWS = (0, 16)
MAX_LEN = 512


def first_key(p, window):
    return max(0, p + 1 - window) if window > 0 else 0


def model_attention(q, k, v, pos, window, scale):
    """the launch's arithmetic for one head: q (rows, hd) rotated fp16 at positions pos .. pos + rows - 1, k / v
    (>= pos + rows, hd) fp16 cache rows.  fp32 scores, the scale applied in fp32, key tiles of 64 at absolute positions,
    online softmax per row in fp32, P rounded to fp16 for P V, fp32 accumulation, one fp16 rounding -> (rows, hd) fp16"""
    q32, k32, v32 = (np.asarray(t, dtype=np.float16).astype(np.float32) for t in (q, k, v))
    rows, hd = q32.shape
    scale = np.float32(scale)
    p = pos + np.arange(rows)
    lo = np.array([first_key(int(x), window) for x in p])
    m = np.full(rows, -np.inf, dtype=np.float32)
    l = np.zeros(rows, dtype=np.float32)
    acc = np.zeros((rows, hd), dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for j in range(int(lo.min()) // TILE, int(p.max()) // TILE + 1):
            keys = np.arange(TILE * j, TILE * j + TILE)
            kt = np.zeros((TILE, hd), dtype=np.float32)
            vt = np.zeros((TILE, hd), dtype=np.float32)
            ok = keys <= p.max()
            kt[ok], vt[ok] = k32[keys[ok]], v32[keys[ok]]
            s = (q32 @ kt.T).astype(np.float32) * scale
            mask = (keys[None, :] <= p[:, None]) & (keys[None, :] >= lo[:, None])
            s = np.where(mask, s, -np.inf).astype(np.float32)
            mn = np.maximum(m, s.max(axis=1))
            ms = np.where(np.isneginf(mn), np.float32(0), mn).astype(np.float32)
            cf = np.exp((m - ms).astype(np.float32)).astype(np.float32)
            pr = np.exp((s - ms[:, None]).astype(np.float32)).astype(np.float32)
            l = (l * cf + pr.sum(axis=1, dtype=np.float32)).astype(np.float32)
            acc = (acc * cf[:, None] + pr.astype(np.float16).astype(np.float32) @ vt).astype(np.float32)
            m = mn
    return (acc / l[:, None]).astype(np.float16)


def exact_attention(q, k, v, pos, window, scale):
    """float64 softmax attention on the same fp16 operands -> ((rows, hd) float64, max|v| over each row's keys)"""
    q64, k64, v64 = (np.asarray(t, dtype=np.float16).astype(np.float64) for t in (q, k, v))
    rows = q64.shape[0]
    out = np.empty_like(q64)
    vmax = np.empty(rows)
    for i in range(rows):
        p = pos + i
        a = first_key(p, window)
        s = (k64[a:p + 1] @ q64[i]) * float(np.float32(scale))
        w = np.exp(s - s.max())
        out[i] = (w / w.sum()) @ v64[a:p + 1]
        vmax[i] = np.abs(v64[a:p + 1]).max()
    return out, vmax


def error_in_u(got, exact, vmax):
    """max over the rows of |got - exact| in units of u = 2^-11 * max|v| of the row's keys"""
    return float((np.abs(np.asarray(got, dtype=np.float64) - exact).max(axis=1) / (vmax * 2.0 ** -11)).max())


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_entry_and_the_abi_version_moved():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert ENTRY in set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 11


def test_python_binding_covers_the_entry(lib):
    from quip_for_all_amd import capi
    assert ENTRY in capi.SIGNATURES and len(capi.SIGNATURES[ENTRY]) == 17
    assert hasattr(lib, ENTRY)
    assert lib.quip_abi_version() >= 11


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(*, q=p16, out=p16, pos=p16, rows=5, heads=4, kvh=2, hd=64, max_len=32, window=0):
        return lib.quip_rope_attn_chunk_f16(q, p16, p16, p16, p16, pos, p16, p16, out, rows, heads, kvh, hd, max_len,
                                            0.125, window, None)
    assert call(q=None) == -1 and call(out=None) == -1 and call(pos=None) == -1      # QUIP_ERR_NULL_POINTER
    assert call(rows=0) == -2 and call(rows=-3) == -2                                  # QUIP_ERR_BAD_SHAPE
    assert call(max_len=0) == -2
    assert call(heads=6, kvh=4) == -2
    assert call(window=-1) == -2
    assert call(hd=96) == -5 and call(hd=256) == -5                                    # QUIP_ERR_UNSUPPORTED
    assert call(q=p16 + 2) == -3 and call(pos=p16 + 4) == -3                           # QUIP_ERR_MISALIGNED


def test_op_fake_on_meta_tensors():
    import quip_for_all_amd.chunk_attn  # noqa: F401  (defines the op)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    R, H, KVH, HD, L = 7, 8, 2, 64, 40
    out = torch.ops.quip_lib.rope_attn_chunk(m(R, H, HD), m(R, KVH, HD), m(R, KVH, HD), m(L, HD, dtype=torch.float32),
                                             m(L, HD, dtype=torch.float32), m(1, dtype=torch.int64), m(KVH, L, HD),
                                             m(KVH, L, HD), 16)
    assert out.device.type == "meta" and tuple(out.shape) == (R, H, HD) and out.dtype == torch.float16


def _stub(head_dim=64):
    from quip_for_all_amd.decode import LlamaShape
    return types.SimpleNamespace(max_len=64, dev=torch.device("cpu"), window=0, _fed=None,
                                 s=LlamaShape(hidden=4 * head_dim, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512))


def test_extend_refuses_what_it_cannot_serve():
    from quip_for_all_amd.batch_decode import BatchDecoder
    from quip_for_all_amd.decode import LlamaDecoder
    with pytest.raises(ValueError, match="empty"):
        LlamaDecoder.extend(_stub(), [])
    with pytest.raises(ValueError, match="empty"):
        LlamaDecoder.extend_graph(_stub(), torch.empty(0, dtype=torch.long))
    with pytest.raises(ValueError, match="chunk"):
        LlamaDecoder.extend(_stub(), [1, 2], chunk=0)
    with pytest.raises(NotImplementedError, match="head_dim"):
        LlamaDecoder.extend(_stub(head_dim=96), [1, 2])
    bd = types.SimpleNamespace(batch=3, dev=torch.device("cpu"))
    for b in (-1, 3):
        with pytest.raises(ValueError, match="slot"):
            BatchDecoder.extend_slot(bd, b, [1, 2])
    with pytest.raises(ValueError, match="tokens"):
        BatchDecoder.extend_slot(bd, 1, [])
    with pytest.raises(RuntimeError, match="append"):
        LlamaDecoder.generate(_stub(), 2, prompt=[1, 2], append=True)


@pytest.mark.parametrize("hd", sorted({s[2] for s in SHAPES}))
@pytest.mark.parametrize("window", WINDOWS)
def test_cpu_model_of_the_arithmetic_stays_inside_the_bound(hd, window):
    """every (rows, pos) of the GPU test, normal data and keys scaled up to 3 x (sharper softmax, larger scores)"""
    rng = np.random.default_rng(100 * hd + window)
    worst = 0.0
    for rows, pos in CHUNKS:
        for kscale in (1.0, 3.0):
            n = pos + rows
            q = rng.standard_normal((rows, hd)).astype(np.float16)
            k = (kscale * rng.standard_normal((n, hd))).astype(np.float16)
            v = rng.standard_normal((n, hd)).astype(np.float16)
            scale = 1.0 / np.sqrt(hd)
            exact, vmax = exact_attention(q, k, v, pos, window, scale)
            e = error_in_u(model_attention(q, k, v, pos, window, scale), exact, vmax)
            print(f"hd {hd} window {window} rows {rows} pos {pos} k x{kscale}: {e:.3f} u")
            worst = max(worst, e)
    assert worst <= BOUND_U
