"""The grouped skinny product (csrc/e8p_skinny_group.hip, quip_lib::mm_skinny_group): 1..3 matrices of one codebook, M <= 32
and k in one launch -- bit for bit the single launches, inside the single launch's bound against float64 -- and the
QUIP_SKINNY_GROUP route of forward_group: a batched decode step with the switch on gives the bits of the switch off."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CODES = {"E8P12": (torch.int16, 8, 1), "E8P12RVQ4B": (torch.int32, 8, 1), "E8P12RVQ3B": (torch.int32, 32, 3),
         "D4": (torch.uint8, 4, 1), "HI": (torch.int32, 8, 1)}       # code dtype, in features per code column (num, den)


@functools.lru_cache(maxsize=None)
def _codebook(cbid):
    import quip_for_all_amd as Q
    return Q.codebook.codebook_id[cbid](inference=True).to(DEV)


@functools.lru_cache(maxsize=None)
def _problems(cbid, ns, k):
    """seeded random codes of (n, k) matrices and their dense float64 weights (every bit pattern is a code)"""
    dtype, num, den = CODES[cbid]
    rng = np.random.default_rng(sum(ns) + k)
    qs = [torch.from_numpy(rng.integers(0, 256, (n, k * den // num * dtype.itemsize), dtype=np.uint8)).view(dtype).to(DEV)
          for n in ns]
    return qs, [_codebook(cbid).decompress_weight(q).double() for q in qs]


def _xs(M, k, count, seed, same=False):
    rng = np.random.default_rng(seed)
    xs = [torch.from_numpy(rng.standard_normal((M, k)).astype(np.float16)).to(DEV) for _ in range(1 if same else count)]
    return xs * count if same else xs


def _check(cbid, ns, k, M, same=False):
    cb = _codebook(cbid)
    qs, Ws = _problems(cbid, ns, k)
    xs = _xs(M, k, len(ns), M + k, same)
    assert cb.skinny_group_supported(M, list(ns), k) == (max(ns) < 11008)      # (two column blocks: served, not routed)
    ys = cb.mm_skinny_group(xs, qs)
    assert len(ys) == len(ns)
    for x, q, W, y, n in zip(xs, qs, Ws, ys, ns):
        assert y.shape == (M, n) and y.dtype == torch.float16
        assert torch.equal(y, cb.mm_skinny(x, q)), "the single launch's bits"
        z64 = x.double() @ W.T
        tol = 2.0 ** -10 * z64.abs() + 2.0 ** -21 * (x.double().abs() @ W.abs().T) + 1e-7
        assert bool(((y.double() - z64).abs() <= tol).all())


# one partial column block; the tile table across problems; at K = 384 more tiles than CUs with one column block per
# workgroup (288) and with two (344, a partial last block)
SHAPES = [(ns, k) for k in (128, 384, 2176, 4096) for ns in ((34,), (512, 128, 128))] + \
         [((4096, 4096, 1024), 384), ((11008, 11008), 384)]


@pytest.mark.parametrize("M", [2, 16, 17, 31, 32])
@pytest.mark.parametrize("ns,k", SHAPES)
def test_group_equals_single_launches_and_float64_e8p12(ns, k, M):
    """K = 128: one unit, fifteen idle waves; 384: fewer units than slices; 2176: 17 units, one slice a unit longer; M on
    both sides of the 16-row staging, rows >= M re-reading row M - 1.  M = 17 passes ONE x tensor for every problem."""
    _check("E8P12", ns, k, M, same=(M == 17))


@pytest.mark.parametrize("M", [16, 31])
@pytest.mark.parametrize("k", [384, 2176])
@pytest.mark.parametrize("cbid", ["E8P12RVQ4B", "E8P12RVQ3B", "D4", "HI"])
def test_group_equals_single_launches_and_float64_other_codebooks(cbid, k, M):
    _check(cbid, (512, 128, 128), k, M)


def test_group_is_stable_and_rows_do_not_depend_on_the_batch():
    cb = _codebook("E8P12")
    qs, _ = _problems("E8P12", (4096, 4096, 1024), 384)
    xs = _xs(16, 384, 3, 5)
    first = cb.mm_skinny_group(xs, qs)
    for _ in range(4):
        again = cb.mm_skinny_group(xs, qs)
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    rows = cb.mm_skinny_group([x[3:5].contiguous() for x in xs], qs)
    assert all(torch.equal(a[3:5], b) for a, b in zip(first, rows))


def test_group_refusals_launch_nothing():
    """mixed column tiling, M = 33, four problems, unequal K: the op raises and names the field; the C entry answers a
    status and leaves the outputs alone"""
    from quip_for_all_amd import capi
    cb = _codebook("E8P12")
    grid = cb.grid_packed_abs
    q = {(n, k): torch.zeros(n, k // 8, dtype=torch.int16, device=DEV) for n, k in ((4096, 128), (11008, 128), (64, 256))}
    x = {(m, k): torch.zeros(m, k, dtype=torch.float16, device=DEV) for m, k in ((8, 128), (33, 128), (8, 256))}
    op = torch.ops.quip_lib.mm_skinny_group
    assert not cb.skinny_group_supported(8, [4096, 11008], 128)
    for xs, qs, field in (([x[8, 128]] * 2, [q[4096, 128], q[11008, 128]], "column tiling"),
                          ([x[33, 128]], [q[4096, 128]], "M = 33"),
                          ([x[8, 128]] * 4, [q[4096, 128]] * 4, "1..3 problems"),
                          ([x[8, 128], x[8, 256]], [q[4096, 128], q[64, 256]], "x: every problem needs the same")):
        with pytest.raises(ValueError, match=field):
            op(xs, qs, 0, grid, None, 0.0)
    ys = [torch.full((33, 11008), 7.0, dtype=torch.float16, device=DEV) for _ in range(4)]
    arr = ctypes.c_void_p * 4
    stream = torch.cuda.current_stream().cuda_stream
    for ns, m in (((4096, 11008), 8), ((4096,), 33), ((4096,) * 4, 8)):
        status = capi.lib().quip_mm_skinny_group_f16(
            0, arr(*[x[8, 128].data_ptr()] * 4), arr(*[q[n, 128].data_ptr() for n in ns]), arr(*[y.data_ptr() for y in ys]),
            (ctypes.c_int32 * 4)(*ns), len(ns), m, 128, grid.data_ptr(), None, 0.0, stream)
        assert status in (-2, -5), (ns, m, status)      # QUIP_ERR_BAD_SHAPE, QUIP_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool((y == 7.0).all()) for y in ys)


def _decode_run(dec, B, calls):
    from tests.test_gpu_batch_decode import _prompts
    bd = dec.batched(B)
    prompts = _prompts(dec.s.vocab, tuple(range(1, B + 1)), seed=3)
    calls.clear()
    eager = bd.generate(prompts, 4, use_graph=False)
    out = [eager, bd.step_logits.clone(), bd.kcache.clone(), bd.vcache.clone(), bd.generate(prompts, 4), bd.step_logits.clone()]
    return bd.regimes(), len(calls), out


@pytest.mark.parametrize("cbid", ["E8P12", "E8P12RVQ4B"])
def test_route_gives_the_bits_of_the_per_module_route(cbid, monkeypatch):
    """2-layer 4096-wide decoder, B = 8 (all seven modules skinny_fp16): four eager steps and a captured replay with
    QUIP_SKINNY_GROUP on -- q / k / v and gate / up through mm_skinny_group -- give the tokens, logits and cache rows of
    the switch off.  B = 3 (rows_exact) keeps the old route with the switch on."""
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=4096, ffn=11008, layers=2, heads=32, kv_heads=32, vocab=1024)
    np.random.seed(13)
    dec = D.LlamaDecoder(shape, cbid, max_len=32, device=DEV, seed=4, device_init=True)
    cbt = type(dec.layers[0]["q"].codebook)
    calls, inner = [], cbt.mm_skinny_group
    monkeypatch.setattr(cbt, "mm_skinny_group", lambda self, xs, qs: (calls.append(len(qs)), inner(self, xs, qs))[1])
    for B, regime in ((8, "skinny_fp16"), (3, "rows_exact")):
        monkeypatch.delenv("QUIP_SKINNY_GROUP", raising=False)
        regimes, n_off, off = _decode_run(dec, B, calls)
        # (B = 8: all seven modules; B = 3: the grouped ones -- down_proj's k = 11008 is past one rows-mode pass there)
        assert {regimes[m] for m in (regimes if B == 8 else ("q", "k", "v", "gate", "up"))} == {regime}, regimes
        monkeypatch.setenv("QUIP_SKINNY_GROUP", "1")
        _, n_on, on = _decode_run(dec, B, calls)
        assert n_off == 0 and (n_on > 0) == (B == 8), (B, n_off, n_on)
        for a, b in zip(off, on):
            assert torch.equal(a, b)
