"""Speculative greedy decode without a GPU: the C ABI of the two launches (declared, bound, exported, operands refused
before any launch), the ops' fakes and their CPU refusal, the restatement of the function on lists (spec.accept_draft_ref)
on hand-written cases with known answers, one per clause of DESIGN 4.18, and the build-time invariant of the kernels: no
scratch, and exactly the LDS the header derives (the suffix and the wave partials of the key)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("quip_spec_draft_i64", "quip_spec_accept_draft_i64")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_and_binding_hold_both_symbols_and_the_abi_moved(lib):
    from quip_for_all_amd import capi
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    assert abi >= 22 and lib.quip_abi_version() == abi
    for name, nargs in zip(NAMES, (13, 18)):
        assert name in declared and name in capi.SIGNATURES and len(capi.SIGNATURES[name]) == nargs and hasattr(lib, name)
        decl = re.search(name + r"\s*\(([^)]*)\)", src).group(1)
        assert len(decl.split(",")) == nargs


def test_operands_are_refused_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    draft, accept = lib.quip_spec_draft_i64, lib.quip_spec_accept_draft_i64
    # (rows_tok, n_draft, pos, hist, hist_cap, pred, n_pred, pred_cap, stats, k, gmin, gmax, stream)
    good = [p, p, p, p, 64, p, p, 8, p, 4, 1, 3, None]

    def d(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return draft(*a)
    for i in (0, 1, 2, 3, 6, 8):
        assert d(**{f"a{i}": None}) == -1                                    # a null operand
    assert d(a5=None) == -1                                                  # pred: null only where pred_cap is 0
    for i in (0, 2, 3, 5, 8):
        assert d(**{f"a{i}": p + 4}) == -3                                   # int64 operands: 8 bytes
    for i in (1, 6):
        assert d(**{f"a{i}": p + 2}) == -3                                   # int32 operands: 4 bytes
    for kw in (dict(a9=0), dict(a9=16), dict(a10=-1), dict(a10=4), dict(a11=9), dict(a4=0), dict(a7=-1),
               dict(a4=(1 << 20) - 7)):
        assert d(**kw) == -2, kw                                             # k, ngram, capacities
    # (argmax, lse, rows_tok, n_draft, pos, hist, hist_cap, pred, n_pred, pred_cap, out, out_len, cap_out, stats, k, gmin,
    #  gmax, stream)
    good2 = [p, p, p, p, p, p, 64, p, p, 8, p, p, 16, p, 4, 1, 3, None]

    def a(**kw):
        v = list(good2)
        for i, x in kw.items():
            v[int(i[1:])] = x
        return accept(*v)
    for i in (0, 1, 2, 3, 4, 5, 8, 11, 13):
        assert a(**{f"a{i}": None}) == -1
    assert a(a7=None) == -1 and a(a10=None) == -1                            # pred / out: null only with capacity 0
    for i in (0, 2, 4, 5, 7, 10, 11, 13):
        assert a(**{f"a{i}": p + 4}) == -3
    for i in (1, 3, 8):
        assert a(**{f"a{i}": p + 2}) == -3
    for kw in (dict(a14=0), dict(a14=16), dict(a15=-1), dict(a15=4), dict(a16=9), dict(a6=0), dict(a9=-1), dict(a12=-1),
               dict(a6=1 << 20)):
        assert a(**kw) == -2, kw


def test_fakes_and_cpu_refusal():
    import quip_for_all_amd.spec  # noqa: F401  (defines the ops)

    def m(n, dt=torch.int64, device="meta"):
        return torch.zeros(n, dtype=dt, device=device)
    for device in ("meta", "cpu"):
        args = (m(5, device=device), m(1, torch.int32, device), m(1, device=device), m(64, device=device), m(8, device=device),
                m(1, torch.int32, device), m(4, device=device), 1, 3)
        args2 = (m(5, device=device), m(5, torch.float32, device), args[0], args[1], args[2], args[3], args[4], args[5],
                 m(16, device=device), m(1, device=device), args[6], 1, 3)
        if device == "meta":
            assert torch.ops.quip_lib.spec_draft(*args) is None
            assert torch.ops.quip_lib.spec_accept_draft(*args2) is None
        else:
            with pytest.raises((NotImplementedError, RuntimeError)):         # no CPU kernel, no fallback
                torch.ops.quip_lib.spec_draft(*args)
            with pytest.raises((NotImplementedError, RuntimeError)):
                torch.ops.quip_lib.spec_accept_draft(*args2)


def test_the_decoder_has_the_method():
    from quip_for_all_amd.decode import LlamaDecoder
    assert callable(LlamaDecoder.generate_speculative)


# ---- accept_draft_ref on cases with known answers ------------------------------------------------------------------------
def _state(rows, n_draft, p0, text, pred=(), k=None, cap_out=8, out=(), stats=(0, 0, 0, 0)):
    """a state after a pass at p0: hist[0 .. p0] = text, hist[p0] == rows[0]"""
    k = len(rows) - 1 if k is None else k
    assert len(text) == p0 + 1 and text[-1] == rows[0]
    hist = list(text) + [-7] * (k + 3)
    o = list(out) + [-9] * (cap_out - len(out))
    return dict(rows_tok=list(rows), n_draft=n_draft, pos=p0 + k + 1, hist=hist, pred=list(pred), out=o, out_len=len(out),
                stats=list(stats))


def test_ref_accepts_the_confirmed_prefix_and_emits_it():
    from quip_for_all_amd.spec import accept_draft_ref
    # rows: current 5, guesses 6 7 8 (k = 4, one row of padding); the model says 6 7 9 . .: two guesses stand, t = 9
    st = _state([5, 6, 7, 8, 0], 3, 2, [1, 2, 5], out=[4])
    new = accept_draft_ref(st, [6, 7, 9, 3, 3], [0.5] * 5, 4, 1, 3)
    assert new["out"][:4] == [4, 6, 7, 9] and new["out_len"] == 4 and new["out"][4:] == [-9] * 4
    assert new["hist"][:6] == [1, 2, 5, 6, 7, 9] and new["hist"][6] == -7 and new["pos"] == 5
    assert new["stats"] == [1, 3, 2, 0]
    assert new["rows_tok"] == [9, 0, 0, 0, 0] and new["n_draft"] == 0      # 9 never occurred: nothing to draft
    assert st["out_len"] == 1 and st["pos"] == 7                            # the argument is left alone
    # all guesses stand; a guess beyond n_draft is never looked at (row 4 is padding: 0 == argmax[3] proves nothing)
    new = accept_draft_ref(st, [6, 7, 8, 0, 3], [0.5] * 5, 4, 1, 3)
    assert new["out"][:5] == [4, 6, 7, 8, 0] and new["stats"] == [1, 3, 3, 0] and new["pos"] == 6
    # the first guess already fails
    new = accept_draft_ref(st, [2, 7, 8, 0, 3], [0.5] * 5, 4, 0, 0)
    assert new["out"][:2] == [4, 2] and new["stats"] == [1, 3, 0, 0] and new["pos"] == 3 and new["rows_tok"] == [2, 0, 0, 0, 0]
    # out at capacity: the writes are dropped, the count goes on
    st = _state([5, 6, 7, 8, 0], 3, 2, [1, 2, 5], out=[4, 4], cap_out=3)
    new = accept_draft_ref(st, [6, 7, 9, 3, 3], [0.5] * 5, 4, 1, 3)
    assert new["out"] == [4, 4, 6] and new["out_len"] == 5


def test_ref_non_finite_rows():
    from quip_for_all_amd.spec import accept_draft_ref
    st = _state([5, 6, 7, 8, 0], 3, 2, [1, 2, 5], out=[4])
    for bad in (NAN, INF, -INF):
        new = accept_draft_ref(st, [6, 7, 9, 3, 3], [bad, 0.5, 0.5, 0.5, 0.5], 4, 1, 3)     # row 0: nothing but the flag
        assert new["stats"] == [0, 0, 0, 1] and new["pos"] == 2
        assert {k: v for k, v in new.items() if k not in ("stats", "pos")} == \
            {k: v for k, v in st.items() if k not in ("stats", "pos")}
        # row a = 2 would give t: its lse is not finite, so the prefix ends one earlier and t is row 1's arg-max
        new = accept_draft_ref(st, [6, 7, 9, 3, 3], [0.5, 0.5, bad, 0.5, 0.5], 4, 1, 3)
        assert new["out"][:3] == [4, 6, 7] and new["stats"] == [1, 3, 1, 0] and new["pos"] == 4
        assert new["hist"][:5] == [1, 2, 5, 6, 7]


def test_ref_draft_three_key_order():
    from quip_for_all_amd.spec import draft_ref
    #        0  1  2  3  4  5  6  7  8  9 10 11
    text = [1, 2, 3, 9, 2, 3, 8, 3, 7, 1, 2, 3]
    # suffix (1 2 3) occurs at e = 2 only besides itself: the longest match beats the more recent (2 3) at e = 5 and (3) at 7
    assert draft_ref(text, 11, [], 4, 1, 3) == [9, 2, 3, 8]
    assert draft_ref(text, 11, [], 4, 1, 2) == [8, 3, 7, 1]                 # gmax = 2: (2 3) at e = 2 and e = 5, the later wins
    assert draft_ref(text, 11, [], 4, 1, 1) == [7, 1, 2, 3]                 # gmax = 1: 3 at e = 2, 5, 7; e = 7 has 4 behind it
    assert draft_ref(text, 11, [], 2, 3, 3) == [9, 2]                       # k cuts the continuation
    assert draft_ref(text, 11, [], 4, 4, 8) == []                           # nothing of length >= 4
    # the fullest continuation beats the most recent: 3 at e = 2 has 4 tokens behind it, 3 at e = 5 only 1
    assert draft_ref([7, 5, 3, 1, 1, 3, 3], 6, [], 4, 1, 1) == [1, 1, 3, 3]
    assert draft_ref([7, 5, 3, 1, 1, 3, 3], 6, [], 1, 1, 1) == [3]          # k = 1: both are full, the later one wins
    # a suffix longer than the text so far is skipped, shorter ones still count
    assert draft_ref([4, 4], 1, [], 4, 1, 8) == [4]
    assert draft_ref([4], 0, [], 4, 1, 8) == []                             # e < len(C) - 1: a token is no match of itself


def test_ref_draft_seam_overlap_and_gmax_zero():
    from quip_for_all_amd.spec import draft_ref
    # a match may not straddle the seam: pred ends in 1, the text starts with 2; suffix (1 2) is found nowhere in one piece
    assert draft_ref([2, 5, 1, 2], 3, [6, 1], 4, 2, 2) == []
    assert draft_ref([2, 5, 1, 2], 3, [6, 1], 4, 1, 2) == [5, 1, 2]         # ... but (2) at e = 2 (text index 0) is
    # a continuation does not cross it either: (1) at the end of pred has nothing behind it in pred
    assert draft_ref([2, 5, 1], 2, [6, 1], 4, 1, 1) == []
    assert draft_ref([2, 5, 1], 2, [1, 6], 4, 1, 1) == [6]                  # cut by the end of the segment
    # the same match in both: equal length and continuation -> the larger index, the text
    assert draft_ref([1, 8, 5, 1], 3, [1, 7, 7], 2, 1, 1) == [8, 5]
    assert draft_ref([9, 1, 1], 2, [1, 7, 7], 2, 1, 1) == [7, 7]            # ... unless pred's continuation is fuller
    # periodic text drafts itself: the continuation overlaps the suffix
    assert draft_ref([3, 4, 3, 4, 3, 4], 5, [], 6, 2, 2) == [3, 4, 3, 4]    # e = 1 (4 behind it) beats e = 3 (2 behind it)
    assert draft_ref([3, 4, 3, 4, 3, 4], 5, [], 2, 2, 2) == [3, 4]          # k = 2: both are full, the later one wins
    assert draft_ref([3, 4, 3, 4, 3, 4], 5, [], 6, 4, 4) == [3, 4]          # suffix 3 4 3 4 at e = 3 overlaps itself
    assert draft_ref([5, 5, 5, 5], 3, [], 3, 1, 3) == [5]                   # longest match (5 5 5 at e = 2) first
    # gmax = 0: no drafting, whatever repeats
    assert draft_ref([5, 5, 5, 5], 3, [5, 5, 5], 3, 0, 0) == []
    assert draft_ref([5, 5, 5, 5], 3, [5, 5, 5], 3, 0, 1) == draft_ref([5, 5, 5, 5], 3, [5, 5, 5], 3, 1, 1) == [5, 5, 5]


def test_ref_draft_only_and_the_accepted_tokens_are_part_of_the_text():
    from quip_for_all_amd.spec import accept_draft_ref
    st = dict(rows_tok=[2, 0, 0], n_draft=0, pos=3, hist=[1, 2, 3, 2, -7, -7, -7, -7], pred=[], out=[-9] * 4, out_len=0,
              stats=[0, 0, 0, 0])
    new = accept_draft_ref(st, None, None, 2, 1, 3)
    assert new["rows_tok"] == [2, 3, 2] and new["n_draft"] == 2 and new["pos"] == 3 and new["stats"] == [0, 0, 0, 0]
    # the pass confirms both: hist grows by 3 2 and t = 3, and the draft looks the new suffix (2 3 2 3 ...) up in all of it
    new["pos"] += 3
    nxt = accept_draft_ref(new, [3, 2, 3], [0.0, 0.0, 0.0], 2, 1, 3)
    assert nxt["hist"][:7] == [1, 2, 3, 2, 3, 2, 3] and nxt["pos"] == 6 and nxt["out"][:3] == [3, 2, 3]
    assert nxt["rows_tok"] == [3, 2, 3] and nxt["stats"] == [1, 2, 2, 0]


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_spec_kernels_use_no_scratch_and_only_the_suffix_and_the_partials_of_lds():
    from quip_for_all_amd import spec
    hdr = open(os.path.join(REPO, "quip_for_all_amd", "csrc", "spec_rows.hip.h")).read()
    threads = int(re.search(r"constexpr int kSpecThreads = (\d+);", hdr).group(1))
    max_g = int(re.search(r"constexpr int kSpecMaxG = (\d+);", hdr).group(1))
    assert re.search(r"constexpr int kSpecLdsBytes = kSpecMaxG \* 8 \+ \(kSpecThreads / 64\) \* 8;", hdr)
    assert threads == spec.THREADS and max_g == spec.MAX_G
    assert int(re.search(r"constexpr int kSpecMaxK = (\d+);", hdr).group(1)) == spec.MAX_K
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and ("spec_draft_kernel" in name or "spec_accept_draft_kernel" in name)):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(scratch) == 2 and len(lds) == 2, "resource remarks of the two launches not found"
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(v == max_g * 8 + (threads // 64) * 8 for v in lds.values()), lds
