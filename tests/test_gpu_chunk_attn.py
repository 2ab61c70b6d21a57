"""quip_lib::rope_attn_chunk on the device (csrc/chunk_attn.hip.h): accuracy against float64 attention inside the bound of
the CPU model (tests/test_chunk_attn_host.py: 1.5 u, u = 2^-11 max|v| over a row's keys -- derived there, not fitted
to the kernel), cache rows bit identical to the decode launch's, bit-exact invariance under chunking, the causal /
window mask without a tolerance, agreement with the decode launch, the range rule and the op's registration.

Kernel-level worst error seen on an MI355X over all cases below: 0.536 u (bound 1.5 u); against the decode launch
0.685 u (bound 3 u) -- profiles/extend_bench.txt."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_chunk_attn_host import (BOUND_U, CHUNKS, MAX_LEN, SHAPES, WINDOWS, error_in_u, exact_attention, first_key)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 777.0
CASES = [(s, c, w) for s in SHAPES for c in CHUNKS for w in WINDOWS]


def _ops():
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.chunk_attn  # noqa: F401
    return torch.ops.quip_lib


def _make_tables(hd, max_len):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.arange(max_len, dtype=torch.float32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.cos()], -1).to(DEV), torch.cat([ang.sin(), ang.sin()], -1).to(DEV)


@functools.lru_cache(maxsize=None)
def _tables(hd):
    return _make_tables(hd, MAX_LEN)


def _rope(x, cos, sin):
    """the eager formula the launches restate (every operation rounded on its own), x (rows, n, hd) at the tables' rows"""
    d = x.shape[-1] // 2
    rot = torch.cat([-x[..., d:], x[..., :d]], -1)
    return (x.float() * cos[:, None] + rot.float() * sin[:, None]).to(x.dtype)


def _inputs(shape, chunk, seed=0):
    """randn q / k / v of the chunk, caches with randn rows below pos and canaries from pos on"""
    (heads, kvh, hd), (rows, pos) = shape, chunk
    g = torch.Generator().manual_seed(1000 * seed + 10 * rows + pos + hd + heads)
    r = lambda *s: torch.randn(*s, generator=g).to(torch.float16).to(DEV)  # noqa: E731
    q, k, v = r(rows, heads, hd), r(rows, kvh, hd), r(rows, kvh, hd)
    kc, vc = r(kvh, MAX_LEN, hd), r(kvh, MAX_LEN, hd)
    kc[:, pos:], vc[:, pos:] = CANARY, CANARY
    return q, k, v, kc, vc


def _run(q, k, v, kc, vc, pos, window, hd):
    cos, sin = _tables(hd)
    p = torch.tensor([pos], dtype=torch.long, device=DEV)
    return _ops().rope_attn_chunk(q, k, v, cos, sin, p, kc, vc, window)


@functools.lru_cache(maxsize=None)
def _case(shape, chunk, window):
    """one launch on the case's inputs, computed once and shared (read only): inputs, caches before / after, out"""
    q, k, v, kc0, vc0 = _inputs(shape, chunk)
    kc, vc = kc0.clone(), vc0.clone()
    out = _run(q, k, v, kc, vc, chunk[1], window, shape[2])
    torch.cuda.synchronize()
    return dict(q=q, k=k, v=v, kc0=kc0, vc0=vc0, kc=kc, vc=vc, out=out)


@functools.lru_cache(maxsize=None)
def _decoded(shape, chunk, window):
    """the same rows through the decode launch, one position at a time -> (kcache, vcache, out (rows, heads, hd))"""
    (heads, kvh, hd), (rows, pos) = shape, chunk
    c = _case(shape, chunk, window)
    cos, sin = _tables(hd)
    kc, vc = c["kc0"].clone(), c["vc0"].clone()
    outs = []
    for i in range(rows):
        p = torch.tensor([pos + i], dtype=torch.long, device=DEV)
        outs.append(_ops().rope_attn_decode(c["q"][i], c["k"][i], c["v"][i], cos, sin, p, kc, vc, None, window))
    return kc, vc, torch.stack(outs)


def _errors_in_u(shape, chunk, window, got, kc, vc):
    """worst error of `got` (rows, heads, hd) against float64 attention over the rotated q and the given cache rows"""
    (heads, kvh, hd), (rows, pos) = shape, chunk
    c = _case(shape, chunk, window)
    cos, sin = _tables(hd)
    qr = _rope(c["q"], cos[pos:pos + rows], sin[pos:pos + rows]).cpu().numpy()
    kn, vn, gn = kc.cpu().numpy(), vc.cpu().numpy(), got.cpu().numpy()
    worst = 0.0
    for h in range(heads):
        j = h // (heads // kvh)
        exact, vmax = exact_attention(qr[:, h], kn[j], vn[j], pos, window, 1.0 / math.sqrt(hd))
        worst = max(worst, error_in_u(gn[:, h], exact, vmax))
    return worst


@pytest.mark.parametrize("shape,chunk,window", CASES)
def test_accuracy_against_float64_attention(shape, chunk, window):
    c = _case(shape, chunk, window)
    assert torch.isfinite(c["out"]).all()
    e = _errors_in_u(shape, chunk, window, c["out"], c["kc"], c["vc"])
    print(f"shape {shape} chunk {chunk} window {window}: {e:.3f} u (bound {BOUND_U})")
    assert e <= BOUND_U


@pytest.mark.parametrize("shape,chunk,window", CASES)
def test_cache_rows_are_the_decode_launch_rows(shape, chunk, window):
    rows, pos = chunk
    c = _case(shape, chunk, window)
    kcd, vcd, _ = _decoded(shape, chunk, window)
    assert torch.equal(c["kc"], kcd) and torch.equal(c["vc"], vcd)             # appended rows, bit for bit
    for after, before in ((c["kc"], c["kc0"]), (c["vc"], c["vc0"])):
        assert torch.equal(after[:, :pos], before[:, :pos])
        assert torch.equal(after[:, pos + rows:], before[:, pos + rows:])         # canaries
    assert torch.equal(c["vc"][:, pos:pos + rows], c["v"].transpose(0, 1))


@pytest.mark.parametrize("shape,chunk,window", CASES)
def test_agrees_with_the_decode_launch(shape, chunk, window):
    """both are within 1.5 u of the same float64 value (the decode launch keeps P in fp32: its own error is smaller)"""
    c = _case(shape, chunk, window)
    kcd, vcd, outd = _decoded(shape, chunk, window)
    (heads, kvh, hd), (rows, pos) = shape, chunk
    vabs = c["vc"].float().abs()
    worst = 0.0
    for i in range(rows):
        a = first_key(pos + i, window)
        u = vabs[:, a:pos + i + 1].amax(dim=(1, 2)).repeat_interleave(heads // kvh) * 2.0 ** -11      # per head
        d = (c["out"][i].float() - outd[i].float()).abs().amax(dim=1)
        worst = max(worst, float((d / u).max()))
    print(f"shape {shape} chunk {chunk} window {window}: chunk vs decode {worst:.3f} u (bound {2 * BOUND_U})")
    assert worst <= 2 * BOUND_U


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("chunk", [c for c in CHUNKS if c[0] > 1])
@pytest.mark.parametrize("window", WINDOWS)
def test_chunking_invariance(shape, chunk, window):
    rows, pos = chunk
    c = _case(shape, chunk, window)
    for step in (1, 7, 32):
        kc, vc = c["kc0"].clone(), c["vc0"].clone()
        parts = [_run(c["q"][i:i + step], c["k"][i:i + step], c["v"][i:i + step], kc, vc, pos + i, window, shape[2])
                 for i in range(0, rows, step)]
        assert torch.equal(torch.cat(parts), c["out"]), step
        assert torch.equal(kc, c["kc"]) and torch.equal(vc, c["vc"]), step


@pytest.mark.parametrize("shape", SHAPES)
def test_causal_mask_without_tolerance(shape):
    chunk, i = (70, 130), 40
    c = _case(shape, chunk, 0)
    q, k, v = c["q"].clone(), c["k"].clone(), c["v"].clone()
    for t in (q, k, v):
        t[i + 1:] = torch.randn_like(t[i + 1:])
    out = _run(q, k, v, c["kc0"].clone(), c["vc0"].clone(), chunk[1], 0, shape[2])
    assert torch.equal(out[:i + 1], c["out"][:i + 1])
    assert not torch.equal(out[i + 1], c["out"][i + 1])
    # a row's own v is attended to
    v2 = c["v"].clone()
    v2[i] += 8.0
    out = _run(c["q"], c["k"], v2, c["kc0"].clone(), c["vc0"].clone(), chunk[1], 0, shape[2])
    assert torch.equal(out[:i], c["out"][:i])
    assert all(not torch.equal(out[i, h], c["out"][i, h]) for h in range(shape[0]))


@pytest.mark.parametrize("shape", SHAPES)
def test_window_mask_without_tolerance(shape):
    (rows, pos), w, hd = (70, 130), 16, shape[2]
    c = _case(shape, (rows, pos), w)
    # cache rows <= p - w of the FIRST row are outside every row's window
    kc, vc = c["kc0"].clone(), c["vc0"].clone()
    kc[:, :pos - w + 1] = torch.randn_like(kc[:, :pos - w + 1])
    vc[:, :pos - w + 1] = torch.randn_like(vc[:, :pos - w + 1])
    assert torch.equal(_run(c["q"], c["k"], c["v"], kc, vc, pos, w, hd), c["out"])
    # row p - w + 1 is the first row's oldest key
    kc, vc = c["kc0"].clone(), c["vc0"].clone()
    vc[:, pos - w + 1] += 1.0
    out = _run(c["q"], c["k"], c["v"], kc, vc, pos, w, hd)
    assert all(not torch.equal(out[0, h], c["out"][0, h]) for h in range(shape[0]))
    assert torch.equal(out[w:], c["out"][w:])            # rows whose window starts behind it
    # inside the chunk: row i sees chunk rows i - w + 1 .. i
    i = 50
    v2 = c["v"].clone()
    v2[i - w] += 1.0
    k2 = c["k"].clone()
    k2[i - w] = torch.randn_like(k2[i - w])
    out = _run(c["q"], k2, v2, c["kc0"].clone(), c["vc0"].clone(), pos, w, hd)
    assert torch.equal(out[i], c["out"][i]) and torch.equal(out[:i - w], c["out"][:i - w])
    v2 = c["v"].clone()
    v2[i - w + 1] += 1.0
    out = _run(c["q"], c["k"], v2, c["kc0"].clone(), c["vc0"].clone(), pos, w, hd)
    assert all(not torch.equal(out[i, h], c["out"][i, h]) for h in range(shape[0]))
    assert torch.equal(out[i + 1], c["out"][i + 1])      # ... and row i + 1 no longer does


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("bad", ["-1", "max_len - rows + 1", "10 ** 12"])
def test_position_out_of_range(shape, bad):
    rows = 33
    pos = eval(bad, {"max_len": MAX_LEN, "rows": rows})
    q, k, v, kc0, vc0 = _inputs(shape, (rows, 61), seed=1)
    kc, vc = kc0.clone(), vc0.clone()
    out = _run(q, k, v, kc, vc, pos, 0, shape[2])
    assert torch.isnan(out).all()
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    out = _run(q, k, v, kc, vc, MAX_LEN - rows, 0, shape[2])       # the last position that fits
    assert torch.isfinite(out).all()
    assert torch.equal(kc[:, :MAX_LEN - rows], kc0[:, :MAX_LEN - rows])


def test_rows_beyond_one_grid():
    """more query tiles than grid.y holds: the launcher slices the chunk (sliding window: the work stays small)"""
    heads, kvh, hd, w = 1, 1, 64, 16
    rows = 65535 * 64 + 70
    max_len = rows + 8
    cos, sin = _make_tables(hd, max_len)
    g = torch.Generator(device=DEV).manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, device=DEV, dtype=torch.float16)  # noqa: E731
    q, k, v = r(rows, heads, hd), r(rows, kvh, hd), r(rows, kvh, hd)
    kc = torch.full((kvh, max_len, hd), CANARY, dtype=torch.float16, device=DEV)
    vc = kc.clone()
    kc[:, :3], vc[:, :3] = r(kvh, 3, hd), r(kvh, 3, hd)
    pos = torch.tensor([3], dtype=torch.long, device=DEV)
    out = _ops().rope_attn_chunk(q, k, v, cos, sin, pos, kc, vc, w)
    assert torch.equal(vc[0, 3:3 + rows], v[:, 0]) and bool((vc[0, 3 + rows:] == CANARY).all())
    assert torch.equal(kc[0, 3:3 + rows], _rope(k, cos[3:3 + rows], sin[3:3 + rows])[:, 0])
    for lo in (0, 65535 * 64 - 40, rows - 70):          # the first tile, across the seam of the slices, the last rows
        qr = _rope(q[lo:lo + 70], cos[3 + lo:3 + lo + 70], sin[3 + lo:3 + lo + 70])[:, 0].cpu().numpy()
        base = max(0, 3 + lo - w)                       # keys below every window of these rows are not needed
        kn, vn = kc[0, base:3 + lo + 70].cpu().numpy(), vc[0, base:3 + lo + 70].cpu().numpy()
        exact, vmax = exact_attention(qr, kn, vn, 3 + lo - base, w, 1.0 / math.sqrt(hd))
        assert error_in_u(out[lo:lo + 70, 0].cpu().numpy(), exact, vmax) <= BOUND_U


def test_op_registration():
    shape, chunk = SHAPES[0], CHUNKS[1]
    q, k, v, kc, vc = _inputs(shape, chunk)
    cos, sin = _tables(shape[2])
    pos = torch.tensor([chunk[1]], dtype=torch.long, device=DEV)
    torch.library.opcheck(_ops().rope_attn_chunk.default, (q, k, v, cos, sin, pos, kc, vc, 16),
                          test_utils=("test_schema", "test_faketensor"))
