"""quip_lib::rope_attn_decode_batched_start on the device (csrc/decode_glue.hip, StartAttnArgs): the batched decode launch
for sequences whose tokens are cache rows start[b] .. pos[b], row t at rotary position t - start[b] (a left-padded batch).

The oracle is the existing launch, bit for bit: sequence b's own B = 1 slice of rope_attn_decode_batched with
window' = pos + 1 - start (min(window, .) when a window is set) and cos / sin tables whose row pos holds row pos - start
of the real ones.  Both launches then compute the same first key, take the same split decision (on the absolute pos),
walk the same keys in the same lane groups and rotate with the same angles, so the output row and cache row pos of K
and V are equal as bits.  The rows below start are NaN in every test here: a launch that read one would not be finite."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MAX_LEN, B = 512, 4
SHAPES = ((4, 4, 64), (8, 2, 128))                  # heads, kv_heads, head_dim
WINDOWS = (0, 64)
# (pos, start) per sequence.  First batch: no split with a neutral start | split mode, start not a multiple of the lane-group
# count (32 / 16) | split mode with two keys, most splits walk nothing | the last row of the cache.  Second batch: only the
# new row is attended (start == pos) below and above the split threshold, at row 0, and a start just under a window.
BATCHES = (((40, 0), (300, 7), (300, 299), (511, 130)),
           ((200, 200), (300, 300), (0, 0), (256, 200)))
CASES = [(s, w, u, i) for s in SHAPES for w in WINDOWS for u in (False, True) for i in range(len(BATCHES))]


def _ops():
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.batch_decode  # noqa: F401
    return torch.ops.quip_lib


def _workspace(batch, heads, hd):
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    return rope_attn_batched_workspace(batch, heads, hd, DEV)


@functools.lru_cache(maxsize=None)
def _tables(hd):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(MAX_LEN, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    heads, kvh, hd = shape
    g = torch.Generator().manual_seed(17 + hd + 10 * heads + kvh)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.float16).to(DEV)  # noqa: E731
    return r(B, heads, hd), r(B, kvh, hd), r(B, kvh, hd), r(B, kvh, MAX_LEN, hd), r(B, kvh, MAX_LEN, hd)


def _caches(shape, starts):
    """the shared random caches with every row below a sequence's start set to NaN"""
    _, _, _, kc, vc = _inputs(shape)
    kc, vc = kc.clone(), vc.clone()
    for b, s in enumerate(starts):
        if s > 0:
            kc[b, :, :s] = float("nan")
            vc[b, :, :s] = float("nan")
    return kc, vc


def _bits(t):
    return t.contiguous().view(torch.int16)


@functools.lru_cache(maxsize=None)
def _oracle(shape, window, use_ws, batch):
    """per sequence of BATCHES[batch]: (out row, K cache, V cache) of the existing launch on the sequence alone"""
    heads, kvh, hd = shape
    q, k, v, _, _ = _inputs(shape)
    cos, sin = _tables(hd)
    kc0, vc0 = _caches(shape, [s for _, s in BATCHES[batch]])
    ws1 = _workspace(1, heads, hd) if use_ws else None
    ref = []
    for b, (p, s) in enumerate(BATCHES[batch]):
        cos_b, sin_b = cos.clone(), sin.clone()
        cos_b[p], sin_b[p] = cos[p - s], sin[p - s]
        w = p + 1 - s if window == 0 else min(window, p + 1 - s)
        kc1, vc1 = kc0[b:b + 1].clone(), vc0[b:b + 1].clone()
        o = _ops().rope_attn_decode_batched(q[b:b + 1], k[b:b + 1], v[b:b + 1], cos_b, sin_b,
                                            torch.tensor([p], dtype=torch.long, device=DEV), kc1, vc1, ws1, w)
        ref.append((o[0], kc1[0], vc1[0]))
    torch.cuda.synchronize()
    return ref


@pytest.mark.parametrize("shape,window,use_ws,batch", CASES)
def test_equals_the_existing_launch_on_each_sequence_alone(shape, window, use_ws, batch):
    """output and both caches of every sequence, bit for bit; with a workspace three launches in a row on it, and its
    arrival counters back at zero"""
    heads, kvh, hd = shape
    q, k, v, _, _ = _inputs(shape)
    cos, sin = _tables(hd)
    pos = torch.tensor([p for p, _ in BATCHES[batch]], dtype=torch.long, device=DEV)
    start = torch.tensor([s for _, s in BATCHES[batch]], dtype=torch.long, device=DEV)
    ref = _oracle(shape, window, use_ws, batch)
    ws = _workspace(B, heads, hd) if use_ws else None
    for n in range(3 if use_ws else 1):
        kc, vc = _caches(shape, [s for _, s in BATCHES[batch]])
        out = _ops().rope_attn_decode_batched_start(q, k, v, cos, sin, pos, start, kc, vc, ws, window)
        assert torch.isfinite(out).all(), (n, "a row below start was read")
        for b, (o1, kc1, vc1) in enumerate(ref):
            what = (n, b, BATCHES[batch][b])
            assert torch.isfinite(o1).all(), what
            assert torch.equal(_bits(out[b]), _bits(o1)), what
            assert torch.equal(_bits(kc[b]), _bits(kc1)) and torch.equal(_bits(vc[b]), _bits(vc1)), what
    if use_ws:
        assert int(ws[-B * heads * 4:].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("window", WINDOWS)
def test_all_zero_start_is_the_existing_batched_launch(shape, window):
    """no window trick: the same operands through both ops -- output, caches, workspace counters"""
    heads, kvh, hd = shape
    q, k, v, kc0, vc0 = _inputs(shape)
    cos, sin = _tables(hd)
    pos = torch.tensor([40, 300, 255, 511], dtype=torch.long, device=DEV)
    start = torch.zeros(B, dtype=torch.long, device=DEV)
    for use_ws in (False, True):
        ws_a, ws_b = (_workspace(B, heads, hd), _workspace(B, heads, hd)) if use_ws else (None, None)
        ka, va, kb, vb = kc0.clone(), vc0.clone(), kc0.clone(), vc0.clone()
        want = _ops().rope_attn_decode_batched(q, k, v, cos, sin, pos, ka, va, ws_a, window)
        got = _ops().rope_attn_decode_batched_start(q, k, v, cos, sin, pos, start, kb, vb, ws_b, window)
        assert torch.equal(_bits(got), _bits(want)), use_ws
        assert torch.equal(_bits(kb), _bits(ka)) and torch.equal(_bits(vb), _bits(va)), use_ws
        if use_ws:
            assert int(ws_b[-B * heads * 4:].view(torch.int32).abs().sum()) == 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bad", [(300, -1), (300, 301), (MAX_LEN, 7), (40, 41)])
def test_an_idle_sequence_leaves_the_others_alone(shape, bad):
    """start = -1, start = pos + 1 (in split mode and below it) and pos = max_len in place of sequence 1: a NaN row, its
    cache untouched, the other three sequences keep the oracle's bits; twice on one workspace"""
    heads, kvh, hd = shape
    q, k, v, _, _ = _inputs(shape)
    cos, sin = _tables(hd)
    ps = list(BATCHES[0])
    ref = _oracle(shape, 0, True, 0)
    ps[1] = bad
    pos = torch.tensor([p for p, _ in ps], dtype=torch.long, device=DEV)
    start = torch.tensor([s for _, s in ps], dtype=torch.long, device=DEV)
    ws = _workspace(B, heads, hd)
    starts_for_nan = [s for _, s in BATCHES[0]]
    for n in range(2):
        kc, vc = _caches(shape, starts_for_nan)
        kc0, vc0 = kc.clone(), vc.clone()
        out = _ops().rope_attn_decode_batched_start(q, k, v, cos, sin, pos, start, kc, vc, ws, 0)
        assert torch.isnan(out[1]).all(), (n, bad)
        assert torch.equal(_bits(kc[1]), _bits(kc0[1])) and torch.equal(_bits(vc[1]), _bits(vc0[1])), (n, bad)
        for b in (0, 2, 3):
            o1, kc1, vc1 = ref[b]
            assert torch.equal(_bits(out[b]), _bits(o1)), (n, b, bad)
            assert torch.equal(_bits(kc[b]), _bits(kc1)) and torch.equal(_bits(vc[b]), _bits(vc1)), (n, b, bad)
    assert int(ws[-B * heads * 4:].view(torch.int32).abs().sum()) == 0


def test_start_operand_is_checked():
    heads, kvh, hd = SHAPES[0]
    q, k, v, kc0, vc0 = _inputs(SHAPES[0])
    cos, sin = _tables(hd)
    pos = torch.zeros(B, dtype=torch.long, device=DEV)
    for start in (torch.zeros(B, dtype=torch.int32, device=DEV), torch.zeros(B + 1, dtype=torch.long, device=DEV),
                  torch.zeros(B, dtype=torch.long), torch.zeros(2 * B, dtype=torch.long, device=DEV)[::2]):
        with pytest.raises(ValueError, match="start must be"):
            _ops().rope_attn_decode_batched_start(q, k, v, cos, sin, pos, start, kc0.clone(), vc0.clone(), None, 0)
