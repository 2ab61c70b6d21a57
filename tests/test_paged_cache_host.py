"""The paged KV cache without a GPU: PagePool (paged_cache.py) against a straightforward model under a few hundred seeded
random calls, the C ABI of the two paged attention launches (declared, bound, every refusal before any launch) and the
fakes of the two ops."""
import copy
import ctypes
import os
import random
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("quip_rope_attn_decode_paged_f16", "quip_rope_attn_ragged_paged_f16")
PAGE = 64


class Model:
    """the straightforward version: per slot a list of page ids and a length; everything else is recomputed"""

    def __init__(self, n_pages, slots, max_pages):
        self.n_pages, self.max_pages = n_pages, max_pages
        self.pages = [[] for _ in range(slots)]
        self.length = [0] * slots

    def used(self):
        return {p for row in self.pages for p in row}

    def free(self):
        return self.n_pages - len(self.used())

    def reserve_fits(self, slot, length):
        return -(-length // PAGE) - len(self.pages[slot]) <= self.free()

    def fork_fits(self, src, dst):
        if self.length[src] % PAGE == 0:
            return True
        others = {p for b, row in enumerate(self.pages) if b != dst for p in row}
        return self.n_pages - len(others) >= 1


def state(pool):
    return copy.deepcopy((pool.free, pool.ref, pool.table, pool.length))


def check_invariants(pool, handed_out):
    count = [0] * pool.n_pages
    for row in pool.table:
        for p in row:
            if p >= 0:
                count[p] += 1
    assert count == pool.ref                                          # reference count == table entries naming the page
    assert all(count[p] == 0 for p in pool.free)                      # free pages are named by none
    assert len(set(pool.free)) == len(pool.free)
    assert sorted(pool.free) == [p for p in range(pool.n_pages) if count[p] == 0]       # and nothing is lost
    for b, row in enumerate(pool.table):
        held = -(-pool.length[b] // PAGE)
        assert all(p >= 0 for p in row[:held]) and all(p == -1 for p in row[held:])
        j = pool.length[b] // PAGE                                    # the page slot b appends to next is its own
        if j < pool.max_pages and row[j] >= 0:
            assert pool.ref[row[j]] == 1
        assert pool.writable(b)
    assert pool.check()


@pytest.mark.parametrize("seed", (0, 1, 2))
def test_page_pool_against_a_model(seed):
    from quip_for_all_amd.paged_cache import PagePool, PoolExhausted
    rng = random.Random(seed)
    n_pages, slots, max_pages = 9, 4, 6
    pool, model = PagePool(n_pages, slots, max_pages), Model(n_pages, slots, max_pages)
    refused = served = 0
    for _ in range(400):
        op = rng.choice(("reserve", "reserve", "release", "fork"))
        b = rng.randrange(slots)
        before, free_before = state(pool), set(pool.free)
        if op == "reserve":
            length = min(max_pages * PAGE, pool.length[b] + rng.choice((0, 1, 30, 64, 65, 200)))
            fits = model.reserve_fits(b, length)
            try:
                pool.reserve(b, length)
                assert fits
                new = [p for p in pool.table[b] if p >= 0][len(model.pages[b]):]
                assert set(new) <= free_before and len(set(new)) == len(new)          # no page handed out twice
                model.pages[b] += new
                model.length[b] = max(model.length[b], length)
                served += 1
            except PoolExhausted:
                assert not fits
                assert state(pool) == before                          # a refusal changes nothing
                refused += 1
        elif op == "release":
            pool.release(b)
            model.pages[b], model.length[b] = [], 0
        else:
            d = rng.randrange(slots)
            if d == b:
                with pytest.raises(ValueError):
                    pool.fork(b, d)
                continue
            fits = model.fork_fits(b, d)
            try:
                pairs = pool.fork(b, d)
                assert fits
                n = model.length[b]
                shared = model.pages[b][:n // PAGE]
                assert pool.table[d][:len(shared)] == shared
                assert len(pairs) == (1 if n % PAGE else 0)
                if pairs:
                    (sp, dp), = pairs
                    assert sp == model.pages[b][n // PAGE] and dp == pool.table[d][n // PAGE]
                    assert dp not in {p for x, row in enumerate(model.pages) if x != d for p in row}
                model.pages[d] = shared + [dp for _, dp in pairs]
                model.length[d] = n
            except PoolExhausted:
                assert not fits
                assert state(pool) == before
                refused += 1
        assert pool.length == model.length
        assert [[p for p in row if p >= 0] for row in pool.table] == model.pages
        assert pool.free_count() == model.free()
        check_invariants(pool, None)
    assert refused >= 5 and served >= 50                              # both sides of the capacity were exercised


def test_fork_shares_full_pages_and_copies_the_partial_one():
    from quip_for_all_amd.paged_cache import PagePool
    pool = PagePool(12, 3, 6)
    pool.reserve(0, 100)
    pairs = pool.fork(0, 1)
    assert len(pairs) == 1 and pool.table[1][0] == pool.table[0][0] and pool.ref[pool.table[0][0]] == 2    # 1 shared
    assert pairs == [(pool.table[0][1], pool.table[1][1])] and pairs[0][0] != pairs[0][1]                  # 1 copy pair
    assert pool.length[1] == 100 and pool.free_count() == 12 - 3
    pool.release(1)
    pool.reserve(0, 128)
    assert pool.fork(0, 1) == [] and pool.table[1][:2] == pool.table[0][:2] and pool.free_count() == 12 - 2
    assert all(pool.ref[p] == 2 for p in pool.table[0][:2])                                               # 2 shared, no copy
    assert pool.fork(2, 1) == [] and pool.table[1] == [-1] * 6 and pool.length[1] == 0                    # an empty slot
    assert pool.free_count() == 12 - 2
    check_invariants(pool, None)


def test_reserve_refuses_what_no_table_row_holds():
    from quip_for_all_amd.paged_cache import PagePool
    pool = PagePool(4, 2, 2)
    with pytest.raises(ValueError):
        pool.reserve(0, 129)
    with pytest.raises(ValueError):
        pool.reserve(2, 1)
    with pytest.raises(ValueError):
        PagePool(0, 1, 1)


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
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 14


def test_python_binding_covers_both_entries(lib):
    from quip_for_all_amd import capi
    assert len(capi.SIGNATURES[ENTRIES[0]]) == 21 and len(capi.SIGNATURES[ENTRIES[1]]) == 24
    assert all(hasattr(lib, e) for e in ENTRIES)
    assert lib.quip_abi_version() >= 14
    assert set(ENTRIES) <= set(capi.check_symbols())


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def dec(*, q=p16, pos=p16, table=p16, kpool=p16, batch=3, heads=4, kvh=2, hd=64, max_len=384, n_pages=20, max_pages=6,
            window=0, ws=None):
        return lib.quip_rope_attn_decode_paged_f16(q, p16, p16, p16, p16, pos, table, kpool, p16, p16, batch, heads, kvh, hd,
                                                   max_len, n_pages, max_pages, 0.125, window, ws, None)

    def rag(*, q=p16, out=p16, pos=p16, table=p16, slots=(2, 0), seg_rows=(5, 70), rows=None, heads=4, kvh=2, hd=64,
            max_len=384, batch=3, n_pages=20, max_pages=6, window=0):
        n = len(slots)
        sl, sr = (ctypes.c_int32 * n)(*slots), (ctypes.c_int32 * n)(*seg_rows)
        return lib.quip_rope_attn_ragged_paged_f16(q, p16, p16, p16, p16, pos, table, p16, p16, out,
                                                   sum(seg_rows) if rows is None else rows, heads, kvh, hd, max_len, batch,
                                                   n_pages, max_pages, ctypes.addressof(sl), ctypes.addressof(sr), n, 0.125,
                                                   window, None)
    for f in (dec, rag):
        assert f(q=None) == -1 and f(table=None) == -1 and f(pos=None) == -1                      # QUIP_ERR_NULL_POINTER
        assert f(n_pages=0) == -2 and f(max_pages=0) == -2 and f(max_len=0) == -2                 # QUIP_ERR_BAD_SHAPE
        assert f(max_len=385) == -2                                       # more rows of cos / sin than the table addresses
        assert f(heads=6, kvh=4) == -2 and f(window=-1) == -2 and f(batch=0) == -2
        assert f(hd=96) == -5                                                                     # QUIP_ERR_UNSUPPORTED
        assert f(q=p16 + 2) == -3 and f(table=p16 + 2) == -3 and f(pos=p16 + 4) == -3             # QUIP_ERR_MISALIGNED
    assert dec(kpool=None) == -1 and dec(ws=p16 + 4) == -3
    assert dec(max_pages=8193, max_len=64) == -5                          # the table row has to fit the launch's LDS
    assert rag(slots=(2, 2)) == -2 and rag(slots=(2, 3)) == -2 and rag(rows=76) == -2 and rag(seg_rows=(5, 0)) == -2


def test_op_fakes_on_meta_tensors():
    import quip_for_all_amd.paged_attn  # noqa: F401  (defines the ops)
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    R, H, KVH, HD, L, B, NP, MP = 7, 8, 2, 64, 100, 3, 9, 2
    f32, tab = torch.float32, m(B, MP, dtype=torch.int32)
    out = torch.ops.quip_lib.rope_attn_ragged_paged(m(R, H, HD), m(R, KVH, HD), m(R, KVH, HD), m(L, HD, dtype=f32),
                                                    m(L, HD, dtype=f32), m(B, dtype=torch.int64), [2, 0], [4, 3], tab,
                                                    m(NP, KVH, 64, HD), m(NP, KVH, 64, HD), 16)
    assert out.device.type == "meta" and tuple(out.shape) == (R, H, HD) and out.dtype == torch.float16
    out = torch.ops.quip_lib.rope_attn_decode_paged(m(B, H, HD), m(B, KVH, HD), m(B, KVH, HD), m(L, HD, dtype=f32),
                                                    m(L, HD, dtype=f32), m(B, dtype=torch.int64), tab,
                                                    m(NP, KVH, 64, HD), m(NP, KVH, 64, HD), None, 0)
    assert out.device.type == "meta" and tuple(out.shape) == (B, H, HD) and out.dtype == torch.float16


def test_batched_refuses_pages_without_paged():
    from quip_for_all_amd.decode import LlamaDecoder
    with pytest.raises(ValueError, match="pages"):
        LlamaDecoder.batched(object(), 2, pages=4)
