"""The whole token in the persistent launch (csrc/token_tail.hip.h): final RMSNorm, lm_head, arg-max and the next step's
embedding lookup inside the launch of the blocks, against the separate launches on the same inputs.

Bounds are derived, not fitted.  With h the hidden state the blocks-only launch returns (the two launches run the same
block code on the same inputs):
  (a) xnorm_i against float64 x_i = h_i rsqrt(mean(h^2) + eps) w_i:  |xnorm_i - x_i| <= 1/2 ulp16(x_i) + 2^-21 |x_i|
      (one fp16 rounding of a value computed with a handful of fp32 operations; the statistic itself is summed in fp64);
  (b) logit against float64 l = lm_head . xnorm:  |logit - l| <= 1/2 ulp16(l) + D 2^-24 sum_i |W_i xnorm_i|, D = 24 = the
      longest chain of fp32 roundings on the kernel's summation path (token_tail.hip.h, kRoundingChain: 8 dot2 steps of two
      roundings, 2 joins of the four accumulators, 6 steps of the wave reduction), then one fp16 rounding."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D_CHAIN = 24


def _decoder(layers, vocab=32000, g8=False, max_len=48, seed=3, tail=True):
    from quip_for_all_amd import decode as D
    shape = D.LlamaShape(hidden=4096, ffn=14336 if g8 else 11008, layers=layers, heads=32, kv_heads=8 if g8 else 32, vocab=vocab)
    old = {k: os.environ.get(k) for k in ("QUIP_BLOCK_ENGINE", "QUIP_FFN_ENGINE", "QUIP_TOKEN_TAIL")}
    os.environ["QUIP_BLOCK_ENGINE"] = os.environ["QUIP_FFN_ENGINE"] = "1"
    os.environ["QUIP_TOKEN_TAIL"] = "1" if tail else "0"
    np.random.seed(1234 + seed)
    try:
        dec = D.LlamaDecoder(shape, "E8P12", max_len=max_len, device=DEV, seed=seed, device_init=True)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert dec.block_eng and dec.eng_shape == (2 if g8 else 0) and dec.token_tail == tail
    return dec


def _engine_args(dec):
    import math
    return (dec.cos, dec.sin, dec.eng_grid, dec.eng_ws, len(dec.layers), dec.max_len, dec.s.rms_eps,
            1.0 / math.sqrt(dec.s.head_dim), None, -1, dec.eng_codebook, dec.eng_resid_scale, dec.eng_shape,
            getattr(dec, "eng_grid2", None), *((dec.kcache, dec.vcache) if torch.is_tensor(dec.kcache) else (None, None)))


def _blocks_only(dec):
    """h_out of the blocks-only launch at the decoder's current token / position (which it leaves alone)"""
    return torch.ops.quip_lib.block_engine(dec.eng_layers, dec.embed[dec.tok].reshape(-1), dec.pos, *_engine_args(dec))


def _whole_token(dec, lm_head=None, embed=None):
    """the whole-token launch at the decoder's current token / position -> (logits, xnorm); tok / pos are advanced"""
    lm = dec.lm_head if lm_head is None else lm_head
    em = dec.embed if embed is None else embed
    logits = torch.full((1, lm.shape[0]), 7.0, dtype=torch.float16, device=DEV)
    xnorm = torch.zeros(4096, dtype=torch.float16, device=DEV)
    torch.ops.quip_lib.block_engine_token(dec.eng_layers, dec.tok, dec.pos, em, dec.final_norm, lm, logits, *_engine_args(dec),
                                          xnorm)
    return logits, xnorm


def _ulp16(v):
    """the fp16 spacing at |v| (float64 array): 2^(floor(log2 |v|) - 10), 2^-24 below the normal range"""
    e = np.floor(np.log2(np.maximum(np.abs(v), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _check_norm_and_logits(dec, h, logits, xnorm, what):
    h64 = h.double().cpu().numpy().reshape(-1)
    w64 = dec.final_norm.double().cpu().numpy().reshape(-1)
    x64 = h64 / np.sqrt(np.mean(h64 * h64) + dec.s.rms_eps) * w64
    xk = xnorm.double().cpu().numpy()
    ea = np.abs(xk - x64)
    ba = 0.5 * _ulp16(x64) + 2.0 ** -21 * np.abs(x64)
    print(f"{what}: xnorm worst error / bound {np.max(ea / ba):.3f}")
    lm = dec.lm_head
    W = lm.double()
    xg = xnorm.double()
    l64 = (W @ xg).cpu().numpy()
    mag = (W.abs() @ xg.abs()).cpu().numpy()
    lk = logits.double().cpu().numpy().reshape(-1)
    eb = np.abs(lk - l64)
    bb = 0.5 * _ulp16(l64) + D_CHAIN * 2.0 ** -24 * mag
    print(f"{what}: logits worst error / bound {np.max(eb / bb):.3f}")
    assert np.all(ea <= ba), (what, float(np.max(ea / ba)))
    assert np.all(eb <= bb), (what, float(np.max(eb / bb)))
    # report: against the separate launches (F.rms_norm + the dense product) on the same h
    sep = (torch.nn.functional.rms_norm(h.reshape(1, -1), (4096,), dec.final_norm, dec.s.rms_eps) @ lm.T).reshape(-1)
    steps = (np.abs(lk - sep.double().cpu().numpy()) / _ulp16(l64))
    print(f"{what}: {100.0 * np.mean(steps > 0):.3f} % of the logits differ from the separate launches', by at most {steps.max():.1f} fp16 steps")


def test_rounding_chain_is_the_one_stated_next_to_the_code():
    src = open(os.path.join(REPO, "quip_for_all_amd", "csrc", "token_tail.hip.h")).read()
    m = re.search(r"constexpr int kRoundingChain = ([0-9 *+]+);", src)
    assert m and eval(m.group(1)) == D_CHAIN


@pytest.mark.parametrize("layers,vocab,g8", [(1, 32000, False), (32, 32000, False), (1, 128256, True)])
def test_norm_and_logits_within_their_derived_bounds(layers, vocab, g8):
    dec = _decoder(layers, vocab, g8)
    with torch.no_grad():
        for t, tok in enumerate((7, 1234, vocab - 1)):
            dec.tok.fill_(tok)
            dec.pos.fill_(t)
            h = _blocks_only(dec).clone()
            assert int(dec.pos) == t
            logits, xnorm = _whole_token(dec)
            assert dec.engine_status() == 0
            assert int(dec.pos) == t + 1
            assert int(dec.tok) == int(torch.argmax(logits.float()))
            _check_norm_and_logits(dec, h, logits, xnorm, f"{layers} block(s), vocab {vocab}, step {t}")


def test_token_is_the_argmax_of_the_stored_logits_lowest_index_on_ties():
    """duplicated rows of lm_head give bit-equal logits; the duplicate of the winning row sits (i) in the same wave's rows,
    (ii) in another wave of the workgroup, (iii) in another workgroup, (iv) first and last row of the vocabulary"""
    dec = _decoder(1, 32000)
    base = dec.lm_head.clone()
    with torch.no_grad():
        dec.tok.fill_(11)
        dec.pos.fill_(0)
        logits, _ = _whole_token(dec, lm_head=base)
        top = int(torch.argmax(logits.float()))
        assert int(dec.tok) == top and int(dec.pos) == 1
        # vocab 32000 = 256 x 125: workgroup w owns rows [125 w, 125 w + 125), wave v its local rows v, v + 8, ...
        for name, lo, hi in (("one wave", 125 * 40 + 3, 125 * 40 + 19), ("two waves", 125 * 41 + 3, 125 * 41 + 4),
                             ("two workgroups", 125 * 42 + 5, 125 * 200 + 5), ("first and last row", 0, 31999)):
            lm = base.clone()
            lm[lo] = base[top]
            lm[hi] = base[top]
            if top not in (lo, hi):
                lm[top] = 0
            dec.tok.fill_(11)
            dec.pos.fill_(0)
            logits, _ = _whole_token(dec, lm_head=lm)
            lg = logits.reshape(-1)
            assert lg[lo] == lg[hi] == lg.max(), name
            assert int(dec.tok) == lo == int((lg == lg.max()).nonzero()[0]), (name, int(dec.tok), lo, hi)
            assert int(dec.pos) == 1


def test_vocabulary_that_is_not_a_multiple_of_256():
    dec = _decoder(1, 32003)
    with torch.no_grad():
        for t, tok in enumerate((32002, 5)):
            dec.tok.fill_(tok)
            dec.pos.fill_(t)
            h = _blocks_only(dec).clone()
            logits, xnorm = _whole_token(dec)
            assert int(dec.tok) == int(torch.argmax(logits.float())) and int(dec.pos) == t + 1
            _check_norm_and_logits(dec, h, logits, xnorm, f"vocab 32003, step {t}")
        # the last rows belong to the last workgroup: a winner there is found
        lm = dec.lm_head.clone()
        lm[32002] = 4.0 * lm[int(dec.tok)]
        dec.tok.fill_(5)
        dec.pos.fill_(1)
        logits, _ = _whole_token(dec, lm_head=lm)
        assert int(torch.argmax(logits.float())) == int(dec.tok)


def test_two_captured_steps_equal_the_separate_launches_teacher_forced():
    """the second replay reads the embedding row of the token the first one wrote"""
    a = _decoder(2, 32000, tail=True)
    b = _decoder(2, 32000, tail=False)
    assert a._token_tail_on() and not b._token_tail_on()
    a.capture()
    b.capture()
    for dec in (a, b):
        dec.reset(first_token=9)
    first = []
    for t in range(2):
        a.graph.replay()
        b.graph.replay()
        ta, tb = int(a.tok), int(b.tok)
        la = a.step_logits.double().cpu().numpy().reshape(-1)
        lb = b.step_logits.double().cpu().numpy().reshape(-1)
        assert a.engine_status() == 0 and b.engine_status() == 0
        assert int(a.pos) == t + 1 and int(b.pos) == t + 1
        assert ta == int(np.argmax(la)) and tb == int(np.argmax(lb))
        # the same h in both (same block code, same inputs); the two tails round nearly the same sums (report)
        d = np.abs(la - lb) / _ulp16(lb)
        print(f"step {t}: {100.0 * np.mean(d > 0):.3f} % of the logits differ, by at most {d.max():.1f} fp16 steps; tokens {ta} / {tb}")
        # only a tie within one fp16 step of the two top logits may go the other way
        assert ta == tb or abs(lb[ta] - lb[tb]) <= _ulp16(lb[tb:tb + 1])[0], (t, ta, tb, lb[ta], lb[tb])
        first.append(ta)
        b.tok.copy_(a.tok)             # teacher forced: both read the token the whole-token launch wrote
    assert first[0] != 9               # (the second step's embedding row was not the first step's)


def test_a_launch_that_gave_up_answers_nan_token_0_and_the_next_position():
    """workspace word 1 set before the launch (the state 0xE000 leaves behind): every wait still completes -- all workgroups
    are resident -- and the launch answers like the separate launches on an all-NaN hidden state"""
    dec = _decoder(1, 32000)
    with torch.no_grad():
        dec.tok.fill_(21)
        dec.pos.fill_(3)
        dec.eng_ws[4:8].view(torch.int32).fill_(0xE000)
        logits, _ = _whole_token(dec)
        assert bool(torch.isnan(logits).all())
        assert int(dec.tok) == 0 and int(dec.pos) == 4
        assert dec.engine_status() == 0xE000
        dec.engine_reset()
        dec.tok.fill_(21)
        dec.pos.fill_(3)
        h = _blocks_only(dec).clone()
        logits, xnorm = _whole_token(dec)
        assert dec.engine_status() == 0 and int(dec.pos) == 4
        assert int(dec.tok) == int(torch.argmax(logits.float()))
        _check_norm_and_logits(dec, h, logits, xnorm, "after engine_reset")
