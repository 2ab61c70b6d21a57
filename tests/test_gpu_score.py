"""Scoring on the device: quip_lib::nll_rows (csrc/nll_rows.hip.h) against float64 on the same fp16 logits, its rules for
special rows and targets and its bit guarantees; LlamaDecoder.score / perplexity and BatchDecoder.score_slots against the
prompt passes that already exist.

Kernel bound (the issue's, derived there from the order of the sum: at most 594 serial terms per thread + 10 tree levels +
32 units per term, 640 x 2^-24 = 3.8e-5 relative error of the sum = absolute error of its logarithm, rounded up):
  |lse - lse64| <= 1e-4 + 2^-23 |lse64|,   |logprob - logprob64| <= 1e-4 + 2^-22 max(|x_t|, |lse64|).
Model-level comparisons between different but equivalent routes use the project's tolerance for them,
0.03 (max|ref logits| + 1) (tests/test_gpu_extend.py), once for the target logit and once for the log-sum-exp."""
import functools
import os
import subprocess
import sys

import pytest
import torch

from tests.test_gpu_extend import MAX_LEN, _decoder, _fresh, _tokens

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the smallest shapes at which the kernel can go wrong (one group, a tail shorter than a load, misaligned rows of an odd n,
# more than one group per thread, past the registers' 8192 x 4 logits) and the two real vocabularies once each;
# (2, 70001) adds the second read of a long misaligned row
SHAPES = [(1, 1), (3, 7), (2, 255), (5, 257), (4, 1024), (3, 2049), (2, 8193), (2, 32003), (1, 152064), (2, 70001)]
SCALES = (0.0, 1.0, 4.0, 16.0)
P = 45


def _op(logits, target):
    import quip_for_all_amd.score  # noqa: F401  (defines quip_lib::nll_rows)
    return torch.ops.quip_lib.nll_rows(logits, target)


def _logits(rows, n, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, n, generator=g) * scale).half().to(DEV)


def _targets(rows, n, seed):
    g = torch.Generator().manual_seed(seed + 1)
    return torch.randint(0, n, (rows,), generator=g).to(DEV)


def _ref64(logits, target):
    x = logits.double()
    lse = torch.logsumexp(x, -1)
    xt = x.gather(-1, target[:, None])[:, 0]
    return lse, xt, xt - lse


def _within(lp, lse, logits, target):
    lse64, xt, lp64 = _ref64(logits, target)
    e_lse = (lse.double() - lse64).abs()
    e_lp = (lp.double() - lp64).abs()
    b_lse = 1e-4 + 2.0 ** -23 * lse64.abs()
    b_lp = 1e-4 + 2.0 ** -22 * torch.maximum(xt.abs(), lse64.abs())
    print(f"  lse err {float(e_lse.max()):.3e} (bound {float(b_lse.min()):.3e})  logprob err {float(e_lp.max()):.3e} "
          f"(bound {float(b_lp.min()):.3e})")
    return bool((e_lse <= b_lse).all()) and bool((e_lp <= b_lp).all())


@pytest.mark.parametrize("rows,n", SHAPES)
def test_nll_rows_against_float64(rows, n):
    for scale in SCALES:
        logits, target = _logits(rows, n, scale, 1000 * rows + n), _targets(rows, n, n)
        lp, lse, am = _op(logits, target)
        assert lp.dtype == lse.dtype == torch.float32 and am.dtype == torch.int64
        assert tuple(lp.shape) == tuple(lse.shape) == tuple(am.shape) == (rows,)
        print(f"({rows}, {n}) x {scale}:")
        assert _within(lp, lse, logits, target), (rows, n, scale)
        assert torch.equal(am, torch.argmax(logits.float(), -1)), (rows, n, scale)
        lp2, lse2, am2 = _op(logits, target)                                     # two calls: equal bits
        assert torch.equal(lp2.view(torch.int32), lp.view(torch.int32)) and torch.equal(lse2.view(torch.int32), lse.view(torch.int32))
        assert torch.equal(am2, am)


@pytest.mark.parametrize("n", [2049, 8193, 32003, 70001])
def test_argmax_ties_and_the_token_of_argmax_step_batched(n):
    """the maximum planted twice: in two threads of one wave, in two waves, and (n > 8192) in two groups of one thread; the
    first index wins, as torch.argmax and argmax_step_batched have it"""
    import quip_for_all_amd.batch_decode  # noqa: F401  (defines argmax_step_batched)
    pairs = [(8 * 3 + 1, 8 * 5), (8 * 7 + 6, 8 * 70 + 2), (8 * 200 + 7, 8 * 131)]
    if n > 8192:
        pairs.append((4, 8 * 1024))                                              # groups 0 and 1024: both thread 0's
    logits = _logits(len(pairs) + 1, n, 1.0, n)
    for r, (i, j) in enumerate(pairs):
        logits[r, i] = logits[r, j] = 60000.0
    logits[-1] = 0.5                                                             # every entry tied
    _, _, am = _op(logits, _targets(logits.shape[0], n, 3))
    assert am.tolist() == [min(p) for p in pairs] + [0]
    assert torch.equal(am, torch.argmax(logits.float(), -1))
    tok = torch.full_like(am, -5)
    torch.ops.quip_lib.argmax_step_batched(logits, tok, torch.zeros_like(am))
    assert torch.equal(am, tok)


def test_special_rows_follow_the_rules_and_leave_the_others_alone():
    rows, n = 7, 2049                                                            # odd n: every other row is misaligned
    inf, nan = float("inf"), float("nan")
    logits, target = _logits(rows, n, 4.0, 5), _targets(rows, n, 5)
    base = _op(logits, target)
    logits[1, 100], logits[1, 1500] = 65504.0, -65504.0
    logits[2, 3:900:7] = -inf
    logits[3] = -inf
    logits[4, 2000] = nan
    logits[5, 77] = inf
    target[2], target[5] = 4, 78                                                 # finite entries of rows 2 and 5
    target[1] = 100
    lp, lse, am = _op(logits, target)
    for r in (0, 6):                                                             # untouched rows: bit for bit
        assert all(torch.equal(a[r], b[r]) for a, b in zip((lp, lse, am), base)), r
    ok = torch.tensor([0, 1, 2, 6], device=DEV)                                  # finite rows: inside the bound
    assert torch.isfinite(lse[ok]).all() and torch.isfinite(lp[ok]).all()
    assert _within(lp[ok], lse[ok], logits[ok], target[ok])
    assert abs(float(lse[1]) - 65504.0) < 1.0 and int(am[1]) == 100
    assert float(lse[3]) == -inf and torch.isnan(lp[3]) and int(am[3]) == 0      # all -inf
    assert torch.isnan(lse[4]) and torch.isnan(lp[4])                            # one NaN
    assert float(lse[5]) == inf and torch.isnan(lp[5]) and int(am[5]) == 77      # one +inf
    want = torch.logsumexp(logits.float(), -1)                                   # the log-sum-exp is torch's in every case
    assert torch.equal(torch.isnan(lse), torch.isnan(want))
    assert torch.equal(lse[~torch.isnan(lse) & ~torch.isfinite(lse)], want[~torch.isnan(want) & ~torch.isfinite(want)])


@pytest.mark.parametrize("rows,n", [(8, 257), (8, 32003)])
def test_targets_outside_the_row(rows, n):
    logits = _logits(rows, n, 4.0, 9)
    target = torch.tensor([-1, -100, n, n + 5, 0, n - 1, 3, -7], device=DEV)
    lp, lse, am = _op(logits, target)
    assert lp[[0, 1, 7]].view(torch.int32).tolist() == [0, 0, 0]                 # exactly +0.0
    assert torch.isnan(lp[[2, 3]]).all()
    scored = torch.tensor([4, 5, 6], device=DEV)
    assert _within(lp[scored], lse[scored], logits[scored], target[scored])
    assert torch.isfinite(lse).all() and torch.equal(am, torch.argmax(logits.float(), -1))   # written whatever the target


@pytest.mark.parametrize("rows,n", [(3, 2049), (2, 32003), (2, 70001)])
def test_a_row_of_a_call_has_the_bits_of_a_call_on_that_row_alone(rows, n):
    logits, target = _logits(rows, n, 4.0, 17), _targets(rows, n, 17)
    assert any(logits[r].data_ptr() % 16 for r in range(rows))                   # odd n: a row that is not 16-byte aligned
    lp, lse, am = _op(logits, target)
    for r in range(rows):
        alone = logits[r].clone()[None]
        assert alone.data_ptr() % 16 == 0
        lp1, lse1, am1 = _op(alone, target[r:r + 1])
        assert torch.equal(lp1.view(torch.int32), lp[r:r + 1].view(torch.int32)), r
        assert torch.equal(lse1.view(torch.int32), lse[r:r + 1].view(torch.int32)) and torch.equal(am1, am[r:r + 1]), r


# ---- LlamaDecoder.score ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _reference(shape_name):
    """per row t of the P seeded tokens: the logits of a fresh extend(tokens[:t + 1]) -> (float64 log-softmax rows (P, vocab),
    max|logits| per row (P,)); computed once per shape and left unchanged"""
    dec = _fresh(shape_name)
    toks = _tokens(dec, P + 1, 77)
    rows = []
    for t in range(P):
        dec = _fresh(shape_name)
        rows.append(dec.extend(toks[:t + 1])[0].double())
    x = torch.stack(rows)
    _fresh(shape_name)
    return toks, torch.log_softmax(x, -1), x.abs().amax(-1)


def _route_tol(mag):
    return 2 * 0.03 * (mag + 1.0)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
@pytest.mark.parametrize("chunk", [512, 7])
def test_score_values_and_state(shape_name, chunk):
    toks, ref, mag = _reference(shape_name)
    dec = _fresh(shape_name)
    dec.extend(toks[:P], chunk=chunk)
    twin = dec.kcache.clone(), dec.vcache.clone(), dec.pos.clone()
    dec = _fresh(shape_name)
    lp, am = dec.score(toks[:P], toks[1:P + 1], chunk=chunk)
    assert tuple(lp.shape) == tuple(am.shape) == (P,) and lp.dtype == torch.float32 and am.dtype == torch.int64 and lp.is_cuda
    assert torch.equal(dec.kcache, twin[0]) and torch.equal(dec.vcache, twin[1]) and torch.equal(dec.pos, twin[2])
    want = ref.gather(-1, toks[1:P + 1, None])[:, 0]
    err = (lp.double() - want).abs()
    print(f"{shape_name} chunk {chunk}: logprob differs by {float(err.max()):.4f} (tolerance {float(_route_tol(mag).min()):.4f})")
    assert bool((err <= _route_tol(mag)).all())
    # the arg-max is (within the tolerance) the best token of the reference row
    assert bool((ref.amax(-1) - ref.gather(-1, am[:, None])[:, 0] <= _route_tol(mag)).all())
    # the default targets: the list's own next tokens, the last row not scored
    dec = _fresh(shape_name)
    lp_d, am_d = dec.score(toks[:P], chunk=chunk)
    assert torch.equal(lp_d[:-1], lp[:-1]) and float(lp_d[-1]) == 0.0 and torch.equal(am_d, am)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_a_cached_context_conditions_the_scores(shape_name):
    toks, ref, mag = _reference(shape_name)
    dec = _fresh(shape_name)
    dec.extend(toks[:10])
    lp, _ = dec.score(toks[10:30], toks[11:31])
    assert int(dec.pos) == 30
    dec = _fresh(shape_name)
    full, _ = dec.score(toks[:30], toks[1:31])
    tol = _route_tol(mag[10:30])
    assert bool(((lp.double() - full[10:30].double()).abs() <= tol).all())
    assert bool(((lp.double() - ref.gather(-1, toks[1:P + 1, None])[10:30, 0]).abs() <= tol).all())


def test_score_with_the_torch_tail_in_a_fresh_process(tmp_path):
    """QUIP_NLL_ROWS=0 is read once per process, hence the child: it scores the same tokens with the torch expression as the
    tail (the switch as read from the environment) and then, on the same decoder, with the kernel (the module's flag set by
    hand).  Both tails see the same fp16 logits, so they agree within the kernel bound; max(|x_t|, |lse|) >= |logprob| / 2."""
    out = str(tmp_path / "ab.pt")
    code = ("import torch\nfrom quip_for_all_amd import decode as D, score as S\nassert not S._NLL_ROWS\nres = {}\n"
            "for name in ('TINY', 'SMALL'):\n"
            f"    dec = D.LlamaDecoder(getattr(D, name), 'E8P12', max_len={MAX_LEN}, device='{DEV}', seed=3)\n"
            f"    toks = torch.randint(0, dec.s.vocab, ({P + 1},), generator=torch.Generator().manual_seed(77)).to('{DEV}')\n"
            "    for flag in (False, True):\n"
            "        S._NLL_ROWS = flag\n"
            "        dec.reset()\n"
            f"        lp, am = dec.score(toks[:{P}], toks[1:], chunk=7)\n"
            "        res[name, flag] = (lp.cpu(), am.cpu())\n"
            f"torch.save(res, r'{out}')\n")
    env = dict(os.environ, QUIP_NLL_ROWS="0", PYTHONPATH=REPO)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=REPO, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    res = torch.load(out)
    for name in ("TINY", "SMALL"):
        (lp_t, am_t), (lp, am) = res[name, False], res[name, True]
        assert torch.isfinite(lp_t).all() and torch.isfinite(lp).all()
        err = (lp.double() - lp_t.double()).abs()
        bound = 1e-4 + 2.0 ** -22 * lp_t.double().abs() / 2
        print(f"{name}: kernel tail against torch tail, logprob differs by {float(err.max()):.3e}")
        assert bool((err <= bound).all()) and torch.equal(am, am_t)


@pytest.mark.parametrize("shape_name", ["TINY", "SMALL"])
def test_tokens_that_do_not_fit_score_nan(shape_name):
    dec = _fresh(shape_name)
    hist, more = _tokens(dec, 120, 31), _tokens(dec, 21, 32)
    dec.extend(hist)
    k0, v0 = dec.kcache.clone(), dec.vcache.clone()
    lg = dec.extend(more[:20])
    assert torch.isnan(lg).all()
    twin = dec.kcache.clone(), dec.vcache.clone(), dec.pos.clone()
    dec.kcache.copy_(k0)
    dec.vcache.copy_(v0)
    dec.pos.fill_(120)
    lp, am = dec.score(more[:20], more[1:])
    assert torch.isnan(lp).all() and tuple(am.shape) == (20,)
    assert torch.equal(dec.kcache, twin[0]) and torch.equal(dec.vcache, twin[1]) and torch.equal(dec.pos, twin[2])
    assert torch.equal(dec.kcache, k0) and int(dec.pos) == 140                   # (extend's: nothing appended, the counter moves on)
    with pytest.raises(ValueError, match="score"):
        dec.score([])
    with pytest.raises(ValueError, match="targets"):
        dec.score(more[:5], more[:4])


# ---- LlamaDecoder.perplexity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window,stride", [(64, 64), (64, 32), (128, 128)])
def test_perplexity_is_score_over_the_window_plan(window, stride):
    import math
    from quip_for_all_amd.score import plan_score_windows
    dec = _fresh("TINY")
    toks = _tokens(dec, 300, 123)
    got = dec.perplexity(toks, window=window, stride=stride, chunk=50)
    assert sorted(got) == ["argmax_hits", "n_scored", "nll_sum", "ppl"]
    nll, n_scored, hits = 0.0, 0, 0
    for start, length, first in plan_score_windows(300, window, stride):
        dec.pos.zero_()
        lp, am = dec.score(toks[start:start + length], toks[start + 1:start + length + 1], chunk=50)
        nll -= float(lp[first:].double().sum())
        hits += int((am[first:] == toks[start + 1 + first:start + length + 1]).sum())
        n_scored += length - first
    assert got["n_scored"] == n_scored == 299 and got["argmax_hits"] == hits
    assert math.isfinite(got["nll_sum"]) and abs(got["nll_sum"] - nll) <= 1e-12 * abs(nll)
    assert got["ppl"] == math.exp(got["nll_sum"] / got["n_scored"])
    with pytest.raises(ValueError, match="max_len"):
        dec.perplexity(toks, window=MAX_LEN + 1)


# ---- BatchDecoder.score_slots --------------------------------------------------------------------------------------------------
def _state(bd):
    return bd.kcache.clone(), bd.vcache.clone(), bd.tok.clone(), bd.pos.clone()


@pytest.mark.parametrize("chunk", [512, 16])
def test_score_slots_one_slot_is_score_bit_for_bit(chunk):
    dec = _decoder("TINY")
    hist, more = _tokens(dec, 11, 50), _tokens(dec, 45, 51)
    a, b = dec.batched(3), dec.batched(3)
    for bd in (a, b):
        bd.extend_slot(0, _tokens(dec, 5, 52))
        bd.extend_slot(1, hist)
    lp_a, am_a = dec.score(more, chunk=chunk, kv=(a.kcache[:, 1], a.vcache[:, 1]), pos=a.pos[1:2])
    lps, ams = b.score_slots([1], [more], chunk=chunk)
    assert len(lps) == len(ams) == 1 and torch.isfinite(lps[0]).all()
    assert torch.equal(lps[0].view(torch.int32), lp_a.view(torch.int32)) and torch.equal(ams[0], am_a)
    assert torch.equal(b.kcache, a.kcache) and torch.equal(b.vcache, a.vcache)
    assert torch.equal(b.pos, a.pos) and b.pos.tolist() == [5, 56, 0] and torch.equal(b.tok, a.tok)


def test_score_slots_several_slots_against_slot_by_slot():
    """slots (2, 0, 3) get (5, 33, 12) tokens behind positions (0, 11, 7) at chunk 16: the 33-token segment is split over
    passes and pieces of two segments share a pass; slot 1 idles"""
    from quip_for_all_amd.decode import _extend_chunks
    dec = _decoder("TINY")
    slots, lengths, behind, idle = (2, 0, 3), (5, 33, 12), (0, 11, 7), 1
    ref, bd = dec.batched(4), dec.batched(4)
    for d in (ref, bd):
        d.extend_slot(idle, _tokens(dec, 9, 60))
        for b, n in zip(slots, behind):
            if n:
                d.extend_slot(b, _tokens(dec, n, 61 + b))
    k0, v0, tok0, pos0 = _state(bd)
    lists = [_tokens(dec, n, 70 + n) for n in lengths]
    mags = []

    def magnitude(c0, h):
        import torch.nn.functional as F
        lg = F.rms_norm(h, (dec.s.hidden,), dec.final_norm, dec.s.rms_eps) @ dec.lm_head.T
        mags.append(lg.double().abs().amax(-1))
    want = []
    for b, t in zip(slots, lists):                         # the reference: slot by slot (and the size of its logits, on a copy)
        kc, vc, ps = ref.kcache[:, b].clone(), ref.vcache[:, b].clone(), ref.pos[b:b + 1].clone()
        mags.clear()
        _extend_chunks(dec, "reference", t, 16, (kc, vc), ps, magnitude)
        want.append((dec.score(t, chunk=16, kv=(ref.kcache[:, b], ref.vcache[:, b]), pos=ref.pos[b:b + 1]), torch.cat(mags)))
    lps, ams = bd.score_slots(slots, lists, chunk=16)
    assert bd.pos.tolist() == [11 + 33, 9, 5, 7 + 12] and torch.equal(bd.pos, ref.pos) and torch.equal(bd.tok, tok0)
    assert torch.equal(bd.kcache[:, idle], k0[:, idle]) and torch.equal(bd.vcache[:, idle], v0[:, idle])
    for j, n in enumerate(lengths):
        (lp_w, _), mag = want[j]
        assert tuple(lps[j].shape) == tuple(ams[j].shape) == (n,) and float(lps[j][-1]) == 0.0
        err = (lps[j].double() - lp_w.double()).abs()
        print(f"slot {slots[j]}: logprob differs by {float(err.max()):.4f} (tolerance {float(_route_tol(mag).min()):.4f})")
        assert bool((err <= _route_tol(mag)).all()), j


def test_score_slots_refuses_before_anything_is_written():
    dec = _decoder("TINY")
    bd = dec.batched(3)
    bd.extend_slot(0, _tokens(dec, 5, 90))
    before = _state(bd)
    t = _tokens(dec, 6, 91)
    for bad in (lambda: bd.score_slots([1, 1], [t, t]), lambda: bd.score_slots([1, 2], [t]),
                lambda: bd.score_slots([3], [t]), lambda: bd.score_slots([1], [t[:0]]),
                lambda: bd.score_slots([1], [t], chunk=0), lambda: bd.score_slots([1, 2], [t, t], targets=[t, t[:3]])):
        with pytest.raises(ValueError):
            bad()
        assert all(torch.equal(x, y) for x, y in zip(_state(bd), before))
