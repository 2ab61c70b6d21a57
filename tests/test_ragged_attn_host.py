"""The ragged prompt pass without a GPU: the C ABI of the ragged attention launch (declared, bound, every refusal before
any launch), the op's fake, the pass planner of BatchDecoder.extend_slots and what extend_slots / fill_slots refuse."""
import ctypes
import os
import re
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "quip_rope_attn_ragged_f16"
MAX_SEGMENTS = 32


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
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 12
    assert int(re.search(r"#define QUIP_RAGGED_MAX_SEGMENTS (\d+)", src).group(1)) == MAX_SEGMENTS


def test_python_binding_covers_the_entry(lib):
    from quip_for_all_amd import capi, ragged_attn
    assert ENTRY in capi.SIGNATURES and len(capi.SIGNATURES[ENTRY]) == 21
    assert hasattr(lib, ENTRY)
    assert lib.quip_abi_version() >= 12
    assert ragged_attn.MAX_SEGMENTS == MAX_SEGMENTS


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    NOPTR = object()

    def call(*, q=p16, out=p16, pos=p16, cos=p16, kcache=p16, slots=(2, 0, 3), seg_rows=(5, 1, 70), rows=None, heads=4,
             kvh=2, hd=64, max_len=128, batch=5, nseg=None, window=0, slot_ptr=NOPTR, rows_ptr=NOPTR):
        n = max(len(slots), 1)
        sl, sr = (ctypes.c_int32 * n)(*slots), (ctypes.c_int32 * n)(*seg_rows)
        return lib.quip_rope_attn_ragged_f16(
            q, p16, p16, cos, p16, pos, kcache, p16, out, sum(seg_rows) if rows is None else rows, heads, kvh, hd, max_len,
            batch, ctypes.addressof(sl) if slot_ptr is NOPTR else slot_ptr,
            ctypes.addressof(sr) if rows_ptr is NOPTR else rows_ptr, len(slots) if nseg is None else nseg, 0.125, window,
            None)
    # QUIP_ERR_NULL_POINTER, the two host arrays included
    assert call(q=None) == -1 and call(out=None) == -1 and call(pos=None) == -1 and call(kcache=None) == -1
    assert call(slot_ptr=None) == -1 and call(rows_ptr=None) == -1
    # QUIP_ERR_BAD_SHAPE
    assert call(nseg=0) == -2 and call(nseg=-1) == -2
    assert call(slots=tuple(range(33)), seg_rows=(1,) * 33, batch=40) == -2             # more than 32 segments
    assert call(seg_rows=(5, 0, 70)) == -2 and call(seg_rows=(5, -1, 70), rows=74) == -2
    assert call(rows=75) == -2 and call(rows=77) == -2                                    # sum of seg_rows != rows
    assert call(slots=(2, 5, 3)) == -2 and call(slots=(2, -1, 3)) == -2                   # a slot outside [0, batch)
    assert call(slots=(2, 0, 2)) == -2                                                    # a slot named twice
    assert call(heads=6, kvh=4) == -2
    assert call(window=-1) == -2
    assert call(max_len=0) == -2 and call(batch=0) == -2
    # QUIP_ERR_UNSUPPORTED
    assert call(hd=96) == -5 and call(hd=256) == -5
    # QUIP_ERR_MISALIGNED
    assert call(q=p16 + 2) == -3 and call(out=p16 + 8) == -3 and call(cos=p16 + 4) == -3 and call(pos=p16 + 4) == -3


def test_op_fake_on_meta_tensors():
    import quip_for_all_amd.ragged_attn  # noqa: F401  (defines the op)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    R, H, KVH, HD, L, B = 7, 8, 2, 64, 40, 3
    out = torch.ops.quip_lib.rope_attn_ragged(m(R, H, HD), m(R, KVH, HD), m(R, KVH, HD), m(L, HD, dtype=torch.float32),
                                              m(L, HD, dtype=torch.float32), m(B, dtype=torch.int64), [2, 0], [4, 3],
                                              m(B, KVH, L, HD), m(B, KVH, L, HD), 16)
    assert out.device.type == "meta" and tuple(out.shape) == (R, H, HD) and out.dtype == torch.float16


def test_the_op_is_not_in_the_pinned_schema_set():
    from quip_for_all_amd import register_lib
    assert not any("rope_attn_ragged" in str(s) for s in register_lib._SCHEMAS)


LENGTHS = ([1], [5, 70, 64, 1], [600, 3, 515], [17] * 31)


@pytest.mark.parametrize("lengths", LENGTHS, ids=lambda x: f"{len(x)}x{max(x)}")
@pytest.mark.parametrize("chunk", (1, 64, 512))
def test_plan_ragged_passes(lengths, chunk):
    from quip_for_all_amd.batch_decode import plan_ragged_passes
    passes = plan_ragged_passes(lengths, chunk)
    flat = [piece for p in passes for piece in p]
    # coverage exactly once, in order: the pieces of a segment are consecutive and the segments come in order
    want = [(s, t) for s, n in enumerate(lengths) for t in range(n)]
    got = [(s, t) for s, a, r in flat for t in range(a, a + r)]
    assert got == want
    assert all(r >= 1 for _, _, r in flat)
    for p in passes:
        assert len(p) >= 1                                           # no empty pass
        assert sum(r for _, _, r in p) <= chunk                      # budget
        assert len(p) <= MAX_SEGMENTS
        assert len({s for s, _, _ in p}) == len(p)                   # a segment at most once per pass
    # a segment is split only at the budget: every pass but the last is full or holds 32 segments
    for p in passes[:-1]:
        assert sum(r for _, _, r in p) == chunk or len(p) == MAX_SEGMENTS
    assert len(passes) >= -(-sum(lengths) // chunk)


def test_plan_respects_the_segment_limit_and_refuses_a_bad_chunk():
    from quip_for_all_amd.batch_decode import plan_ragged_passes
    passes = plan_ragged_passes([1] * 40, 512)
    assert [len(p) for p in passes] == [32, 8]
    assert plan_ragged_passes([], 8) == [] and plan_ragged_passes([0, 3], 8) == [[(1, 0, 3)]]
    with pytest.raises(ValueError, match="chunk"):
        plan_ragged_passes([3], 0)


def _stub(head_dim=64, batch=3):
    from quip_for_all_amd.decode import LlamaShape
    return types.SimpleNamespace(batch=batch, dev=torch.device("cpu"),
                                 s=LlamaShape(hidden=4 * head_dim, ffn=688, layers=2, heads=4, kv_heads=2, vocab=512))


@pytest.mark.parametrize("method", ("extend_slots", "fill_slots"))
def test_extend_slots_and_fill_slots_refuse_what_they_cannot_serve(method):
    from quip_for_all_amd.batch_decode import BatchDecoder
    f = getattr(BatchDecoder, method)
    with pytest.raises(ValueError, match="duplicate"):
        f(_stub(), [1, 1], [[1, 2], [3]])
    for b in (-1, 3):
        with pytest.raises(ValueError, match="out of range"):
            f(_stub(), [0, b], [[1, 2], [3]])
    with pytest.raises(ValueError, match="empty"):
        f(_stub(), [0, 2], [[1, 2], []])
    with pytest.raises(ValueError, match="mismatch"):
        f(_stub(), [0, 2], [[1, 2]])
    with pytest.raises(NotImplementedError, match="head_dim"):
        f(_stub(head_dim=96), [0, 2], [[1, 2], [3]])


def test_extend_slots_refuses_a_bad_chunk():
    from quip_for_all_amd.batch_decode import BatchDecoder
    with pytest.raises(ValueError, match="chunk"):
        BatchDecoder.extend_slots(_stub(), [0, 2], [[1, 2], [3]], chunk=0)
