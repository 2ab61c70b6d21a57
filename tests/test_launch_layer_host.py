"""Host side of the launch layer (csrc/launch.hip.h, e8p_gemv_v2_plan.hip.h, capi.hip): plans and error codes that are
decided before any launch, so none of this needs a GPU.

The expected values were recorded from the library as it was before the launch layer was factored out (plans: through a
recording hook at the old planners' launch points; codes: from the old entry points) and are held fixed here."""
import ctypes
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, NULL, SHAPE, ALIGN, UNSUPPORTED = 0, -1, -2, -3, -5


@pytest.fixture(scope="module")
def capi():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    assert [capi.lib().quip_strerror(c) for c in (NULL, SHAPE, ALIGN, UNSUPPORTED)] == [
        b"null pointer argument", b"shape not supported by the packed format", b"pointer not 16-byte aligned",
        b"request not supported by this build"]
    return capi


# ---- K-split plans ------------------------------------------------------------------------------------------------------------
def _plans():
    with open(os.path.join(REPO, "tests", "golden", "gemv_v2_plans.json")) as f:
        return json.load(f)


def test_plan_table_covers_both_kernels_and_the_error_rows():
    d = _plans()
    assert d["columns"][-1] == "plan" and len(d["plan_fields"]) == 13
    rows = d["rows"]
    assert len(rows) >= 400
    assert {r[2] for r in rows} == {0, 32, 24, 16, 64, 4, 40}                      # requested table modes
    assert {r[-1][0] for r in rows} == {OK, NULL, UNSUPPORTED}                     # rc
    assert {r[-1][1] for r in rows if r[-1][0] == OK} == {32, 24, 16, 4, 40}        # planned table modes
    assert any(r[-1][3] > 1 for r in rows) and any(r[4] == 1 for r in rows)        # K splits, the blocks = 1 row


def test_plan_hook_reproduces_every_recorded_plan(capi):
    d = _plans()
    from quip_for_all_amd.capi import GEMV_V2_PLAN_FIELDS
    assert list(GEMV_V2_PLAN_FIELDS) == d["plan_fields"]
    bad = []
    for ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws, want in d["rows"]:
        got = capi.gemv_v2_plan(ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws)
        if got != want:
            bad.append(((ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws), want, got))
    assert not bad, "%d of %d plans moved, first: %r" % (len(bad), len(d["rows"]), bad[0])


def test_plan_hook_checks_its_own_pointers(capi):
    out = (ctypes.c_int32 * 13)()
    assert capi.lib().quip_e8p_gemv_v2_plan(None, 1, 4096, 0, 0, 0, 0, 0, 0, 0, 1, out) == NULL
    n = (ctypes.c_int32 * 1)(4096)
    assert capi.lib().quip_e8p_gemv_v2_plan(n, 1, 4096, 0, 0, 0, 0, 0, 0, 0, 1, None) == NULL


# ---- persistent block engine entry points: the order of the checks is observable ------------------------------------------------
@pytest.fixture(scope="module")
def mem():
    buf = (ctypes.c_char * 8192)()
    base = (ctypes.addressof(buf) + 63) & ~63
    return buf, base


def _engine_args(capi, base, **kw):
    a = capi.BlockEngineArgs()
    for i, name in enumerate(("layers", "h_in", "h_out", "pos", "cos", "sin", "grid_packed_abs", "workspace")):
        setattr(a, name, base + 64 * i)
    a.n_layers, a.max_len, a.dbg_layer, a.rms_eps, a.attn_scale = 2, 64, -1, 1e-5, 0.125
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _tail_args(capi, base, a, **kw):
    t = capi.TokenTailArgs()
    for i, name in enumerate(("tok", "embed", "final_norm", "lm_head", "logits")):
        setattr(t, name, base + 1024 + 64 * i)
    t.pos, t.vocab = a.pos, 32000
    for k, v in kw.items():
        setattr(t, k, v)
    return t


# (case, quip_block_engine, quip_block_engine_token): the codes of the entry points before the refactor
ENGINE_CASES = [
    ("null_in", NULL, NULL),
    ("null_layers", NULL, NULL),
    ("misaligned_workspace", ALIGN, ALIGN),
    ("n_layers_0", SHAPE, SHAPE),
    ("shape_3", UNSUPPORTED, UNSUPPORTED),
    ("codebook4_null_grid2", NULL, NULL),
    ("codebook4_misaligned_grid2", ALIGN, ALIGN),
    ("codebook4_null_grid2_shape_3", NULL, UNSUPPORTED),      # the grid2 check sits before / behind the shape dispatch
    ("tail_pos_differs", None, SHAPE),
    ("vocab_255", None, SHAPE),
    ("vocab_255_and_shape_3", None, SHAPE),                   # shape errors before "unsupported"
    ("null_tail", None, NULL),
]


def _engine_case(capi, base, name):
    """-> (in, t) as ctypes pointers or None; t is built for every case (the blocks-only entry point ignores it)"""
    kw, tkw = {}, {}
    if name == "null_layers": kw["layers"] = None
    if name == "misaligned_workspace": kw["workspace"] = base + 64 * 7 + 8
    if name == "n_layers_0": kw["n_layers"] = 0
    if name in ("shape_3", "codebook4_null_grid2_shape_3", "vocab_255_and_shape_3"): kw["shape"] = 3
    if name.startswith("codebook4"): kw["codebook"] = 4
    if name == "codebook4_misaligned_grid2": kw["grid2"] = base + 2048 + 4
    if name == "tail_pos_differs": tkw["pos"] = base + 4096
    if name.startswith("vocab_255"): tkw["vocab"] = 255
    a = _engine_args(capi, base, **kw)
    t = _tail_args(capi, base, a, **tkw)
    return (None if name == "null_in" else ctypes.byref(a)), (None if name == "null_tail" else ctypes.byref(t)), (a, t)


@pytest.mark.parametrize("name,blocks_code,token_code", ENGINE_CASES, ids=[c[0] for c in ENGINE_CASES])
def test_block_engine_entry_points_keep_their_error_codes(capi, mem, name, blocks_code, token_code):
    L = capi.lib()
    pin, pt, keep = _engine_case(capi, mem[1], name)
    if blocks_code is not None:
        assert L.quip_block_engine(pin, None) == blocks_code
    assert L.quip_block_engine_token(pin, pt, None) == token_code
    del keep


# ---- tile / untile: one checked launcher ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["quip_tile_codes", "quip_untile_codes"])
def test_tile_and_untile_check_alike(capi, mem, fn):
    f = getattr(capi.lib(), fn)
    src, dst = mem[1], mem[1] + 4096
    assert f(src, dst, 17, 64, None) == SHAPE                 # rows % 16
    assert f(src, dst, 16, 96, None) == SHAPE                 # row_bytes % 64
    assert f(src, src + 512, 16, 64, None) == UNSUPPORTED     # partial overlap (16 x 64 = 1024 bytes each)
    assert f(src + 512, src, 16, 64, None) == UNSUPPORTED
    assert f(src, src, 16, 64, None) == UNSUPPORTED           # in place
    assert f(src, dst, 0, 64, None) == OK                     # nothing to do: before the alignment and overlap checks
    assert f(src + 8, src + 8, 0, 64, None) == OK
    assert f(src + 8, dst, 16, 64, None) == ALIGN
    assert f(None, dst, 16, 64, None) == NULL and f(src, None, 16, 64, None) == NULL
