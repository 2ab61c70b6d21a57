"""quip_lib::spec_draft / spec_accept_draft on the device against the function on lists (spec.accept_draft_ref): every output
exactly equal -- rows_tok, n_draft, pos, hist, out, out_len, stats -- and the same bits from a second launch on the same
input.  The shapes are the smallest at which the launch can go wrong: every accepted count for k = 1, 4, 7, 15, corpus
lengths around a wave and around the workgroup (spec.THREADS) with the only match on either side of each boundary, the
seam between the prediction and the text, and seeded random corpora over three tokens, where matches abound."""
import random

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
GARBAGE = 77            # what pred holds behind n_pred: never read


def _launch(st, argmax, lse, k, gmin, gmax):
    """the launch on a device copy of the list state `st` -> the state after it, as lists"""
    import quip_for_all_amd.spec  # noqa: F401  (defines the ops)

    def t(v, dt=torch.int64):
        return torch.tensor(v, dtype=dt, device=DEV)
    rows, hist, out, stats = t(st["rows_tok"]), t(st["hist"]), t(st["out"]), t(st["stats"])
    pred = t(list(st["pred"]) + [GARBAGE] * 3)
    n_draft, n_pred = t([st["n_draft"]], torch.int32), t([len(st["pred"])], torch.int32)
    pos, out_len = t([st["pos"]]), t([st["out_len"]])
    if argmax is None:
        torch.ops.quip_lib.spec_draft(rows, n_draft, pos, hist, pred, n_pred, stats, gmin, gmax)
    else:
        torch.ops.quip_lib.spec_accept_draft(t(argmax), t(lse, torch.float32), rows, n_draft, pos, hist, pred, n_pred, out,
                                             out_len, stats, gmin, gmax)
    assert pred.tolist() == list(st["pred"]) + [GARBAGE] * 3 and int(n_pred) == len(st["pred"])
    return dict(rows_tok=rows.tolist(), n_draft=int(n_draft), pos=int(pos), hist=hist.tolist(), pred=list(st["pred"]),
                out=out.tolist(), out_len=int(out_len), stats=stats.tolist())


def _check(st, argmax, lse, k, gmin, gmax):
    """kernel == reference on every field, twice; -> the new state"""
    from quip_for_all_amd.spec import accept_draft_ref
    ref = accept_draft_ref(st, argmax, lse, k, gmin, gmax)
    got = _launch(st, argmax, lse, k, gmin, gmax)
    assert got == ref, (st, argmax, lse, k, gmin, gmax, {f: (got[f], ref[f]) for f in ref if got[f] != ref[f]})
    assert _launch(st, argmax, lse, k, gmin, gmax) == got
    return ref


def _state(rows, n_draft, text, pred=(), cap_out=24, out_len=0, k=None):
    """the list state behind a pass (or, for a draft alone with pos taken back by the caller, in front of one): the text
    so far in hist, its last token in row 0"""
    k = len(rows) - 1 if k is None else k
    assert text[-1] == rows[0]
    return dict(rows_tok=list(rows), n_draft=n_draft, pos=len(text) - 1 + k + 1, hist=list(text) + [-7] * (k + 3),
                pred=list(pred), out=[-9] * cap_out, out_len=out_len, stats=[3, 10, 5, 0])


@pytest.mark.parametrize("k", [1, 4, 7, 15])
def test_every_accepted_count(k):
    text = [40, 41, 42, 43, 40, 41, 50]                   # 40 41 occurs twice: the accepted tokens find something to draft from
    guesses = [40, 41, 42, 43, 40, 41, 42, 43, 40, 41, 42, 43, 40, 41, 42][:k]
    rows = [50] + guesses
    for a in range(k + 1):                                 # the first mismatch at index a (a = k: every guess stands)
        argmax = guesses[:a] + [60 if a < k else 61] + [5] * (k - a)
        new = _check(_state(rows, k, text), argmax, [1.5] * (k + 1), k, 1, 3)
        assert new["stats"] == [4, 10 + k, 5 + a, 0] and new["out_len"] == a + 1 and new["pos"] == len(text) + a
    # fewer guesses than rows: the padding (0) is not a guess even where the model says 0
    for d in range(k):
        rows_d = [50] + guesses[:d] + [0] * (k - d)
        argmax = guesses[:d] + [0] * (k + 1 - d)
        new = _check(_state(rows_d, d, text), argmax, [1.5] * (k + 1), k, 1, 3)
        assert new["stats"][:3] == [4, 10 + d, 5 + d] and new["out_len"] == d + 1


@pytest.mark.parametrize("k", [1, 4, 15])
def test_non_finite_rows_and_out_at_capacity(k):
    text = [40, 41, 42, 43, 40, 41, 50]
    guesses = [40, 41, 42, 43, 40, 41, 42, 43, 40, 41, 42, 43, 40, 41, 42][:k]
    rows, argmax = [50] + guesses, guesses + [9]
    for bad in (NAN, float("inf"), float("-inf")):
        new = _check(_state(rows, k, text), argmax, [bad] + [1.5] * k, k, 1, 3)                 # row 0: the flag alone
        assert new["stats"] == [3, 10, 5, 1] and new["pos"] == len(text) - 1 and new["rows_tok"] == rows
        for a in range(1, k + 1):                                                                # row a: the prefix ends before it
            lse = [1.5] * (k + 1)
            lse[a] = bad
            new = _check(_state(rows, k, text), argmax, lse, k, 1, 3)
            assert new["stats"] == [4, 10 + k, 5 + a - 1, 0]
    for cap_out, out_len in ((0, 0), (1, 0), (k, 0), (k + 1, 0), (6, 5), (6, 6), (6, 9)):        # writes past the end are dropped
        new = _check(_state(rows, k, text, cap_out=cap_out, out_len=out_len), argmax, [1.5] * (k + 1), k, 1, 3)
        assert new["out_len"] == out_len + k + 1


def _only_match(length, at, in_pred):
    """a corpus of `length` tokens, all different but for the last one (the suffix) and the one at index `at`"""
    X = 7
    body = [1000 + i for i in range(length - 1)]
    if at is not None:
        body[at] = X
    return ([X], body) if in_pred else (body + [X], [])


@pytest.mark.parametrize("in_pred", [False, True])
def test_corpus_lengths_around_the_wave_and_the_workgroup(in_pred):
    from quip_for_all_amd.spec import THREADS as T
    k = 4
    for length in (1, 2, 63, 64, 65, T, T + 1, 4 * T + 1):
        last = length - 2 - (1 if in_pred else 0)          # the last end index with a token behind it in its segment
        marks = {0, last}
        for b in (63, 64, 65, T, T + 1, 2 * T, 3 * T, 4 * T):
            marks |= {b - 1, b, b + 1}
        cases = [None] + sorted(m for m in marks if 0 <= m <= last)
        for at in cases:
            text, pred = _only_match(length, at, in_pred)
            st = _state([text[-1]] + [0] * k, 0, text, pred)
            st["pos"] = len(text) - 1
            new = _check(st, None, None, k, 1, 1)
            want = 0 if at is None else min(k, last + 1 - at)
            assert new["n_draft"] == want, (length, at)
        if in_pred and length >= 3:                        # the suffix token as pred's last one: nothing behind it, no candidate
            text, pred = _only_match(length, length - 2, True)
            st = _state([text[-1]] + [0] * k, 0, text, pred)
            st["pos"] = 0
            assert _check(st, None, None, k, 1, 1)["n_draft"] == 0


def test_the_seam_between_prediction_and_text():
    k = 4

    def draft(text, pred, gmin, gmax):
        st = _state([text[-1]] + [0] * k, 0, text, pred)
        st["pos"] = len(text) - 1
        new = _check(st, None, None, k, gmin, gmax)
        return new["rows_tok"][1:1 + new["n_draft"]]
    assert draft([2, 5, 1, 2], [6, 1], 2, 2) == []                    # (1 2) only across the seam
    assert draft([2, 5, 1, 2], [6, 1], 1, 2) == [5, 1, 2]
    assert draft([3, 9, 8, 1, 2], [1, 2, 4, 4], 2, 2) == [4, 4]       # in pred only
    assert draft([1, 2, 4, 3, 1, 2], [9, 9, 9], 2, 2) == [4, 3, 1, 2]  # in the text only
    assert draft([1, 2, 5, 5, 5, 5, 1, 2], [1, 2, 4, 4, 4, 4], 2, 2) == [5, 5, 5, 5]     # in both, equally full: the text
    assert draft([1, 2, 5, 1, 2], [1, 2, 4, 4, 4, 4], 2, 2) == [4, 4, 4, 4]              # in both: pred's is fuller
    assert draft([2, 5, 1], [6, 1], 1, 1) == []                       # pred's last token has no continuation: not across
    assert draft([2, 5, 1], [1, 6], 1, 1) == [6]                      # cut by the end of pred
    assert draft([8, 1, 6, 1], [], 1, 1) == [6, 1]                    # cut by the end of the text
    assert draft([5, 5, 5, 5], [5, 5, 5], 0, 0) == []                 # gmax = 0
    assert draft([3, 4, 3, 4, 3, 4], [], 4, 4) == [3, 4]              # overlap with the suffix
    # g from 1 to 8: a match of exactly g tokens (the token in front of it differs), found with ngram (g, g) and (1, 8),
    # not with (g + 1, 8)
    for g in range(1, 9):
        run = list(range(20, 20 + g))
        text = [90] + run + [70, 71, 72, 73, 74, 91] + run
        assert draft(text, [], g, g) == [70, 71, 72, 73] == draft(text, [], 1, 8)
        if g < 8:
            assert draft(text, [], g + 1, 8) == []
        assert draft([91] + run, [90] + run + [70, 71], g, 8) == [70, 71]


def test_random_corpora_over_three_tokens():
    rng = random.Random(20)
    for case in range(200):
        k = rng.choice([1, 2, 4, 7, 15])
        gmin = rng.randint(0, 3)
        gmax = rng.randint(gmin, 8)
        text = [rng.randrange(3) for _ in range(rng.randint(1, 40))]
        pred = [rng.randrange(3) for _ in range(rng.choice([0, 0, 1, 5, 20]))]
        d = rng.randint(0, k)
        rows = [text[-1]] + [rng.randrange(3) for _ in range(d)] + [0] * (k - d)
        argmax = [r if rng.random() < 0.7 else rng.randrange(3) for r in rows[1:]] + [rng.randrange(3)]
        lse = [NAN if rng.random() < 0.03 else 2.0 for _ in range(k + 1)]
        st = _state(rows, d, text, pred, cap_out=rng.choice([4, 24]), out_len=rng.randint(0, 6))
        new = _check(st, argmax, lse, k, gmin, gmax)
        if case % 4 == 0 and not new["stats"][3]:          # and the draft alone on the state it left
            _check(new, None, None, k, gmin, gmax)


def test_a_position_outside_hist_writes_nothing_but_the_flag():
    k = 4
    st = _state([5, 6, 7, 8, 0], 3, [1, 2, 5])
    for pos in (k, len(st["hist"]) + 1, -3):               # p0 < 0;  p0 + n >= hist_cap;  a negative counter
        bad = dict(st, pos=pos)
        got = _launch(bad, [6, 7, 9, 3, 3], [0.5] * 5, k, 1, 3)
        assert got == dict(bad, stats=[3, 10, 5, 2])
    for pos in (-1, len(st["hist"])):
        bad = dict(st, pos=pos)
        assert _launch(bad, None, None, k, 1, 3) == dict(bad, stats=[3, 10, 5, 2])


def test_operands_are_checked():
    import quip_for_all_amd.spec  # noqa: F401

    def t(n, dt=torch.int64):
        return torch.zeros(n, dtype=dt, device=DEV)
    good = dict(rows_tok=t(5), n_draft=t(1, torch.int32), pos=t(1), hist=t(16), pred=t(4), n_pred=t(1, torch.int32), stats=t(4))
    for name, bad in (("rows_tok", t(1)), ("rows_tok", t(17)), ("rows_tok", t(5, torch.int32)), ("n_draft", t(1)),
                      ("pos", t(2)), ("hist", t(16, torch.int32)), ("pred", t(4).cpu()), ("stats", t(3))):
        with pytest.raises(ValueError, match=name):
            torch.ops.quip_lib.spec_draft(*{**good, name: bad}.values(), 1, 3)
    for ngram in ((2, 1), (0, 9), (-1, 3)):
        with pytest.raises(ValueError, match="gmin"):
            torch.ops.quip_lib.spec_draft(*good.values(), *ngram)
    with pytest.raises(ValueError, match="lse"):
        torch.ops.quip_lib.spec_accept_draft(t(5), t(4, torch.float32), good["rows_tok"], good["n_draft"], good["pos"],
                                             good["hist"], good["pred"], good["n_pred"], t(8), t(1), good["stats"], 1, 3)
