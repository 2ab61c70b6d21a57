"""tests/quantize_hard_cases.py without a GPU: the conditions on the inputs (on the float64 brute force alone), the documented
tie rule as a nearest-point search of its own, the host models of the panels with that rule as the search under the exact step
checker, and the checkers against planted faults."""
import numpy as np
import pytest

from oracle import quip_oracle as O

from tests import ldlq_rvq_cases as R
from tests import quantize_hard_cases as Q

STEPS = [("E8P12", None), ("E8P12RVQ4B", -1.0), ("E8P12RVQ4B", 0.25), ("E8P12RVQ3B", -1.0), ("E8P12RVQ3B", 0.25)]


def test_codebook_facts_the_exactness_rests_on():
    g = O.e8p_full_grid_f64()
    assert np.array_equal(g * 4, np.round(g * 4)) and np.abs(g).min() == 0.25 and np.abs(g).max() == 2.75
    assert (g * g).sum(-1).max() == 16.5
    d2 = ((g[:, None, :] - g[None, :512, :]) ** 2).sum(-1)                     # every codeword against the first 512
    assert d2[d2 > 0].min() == 2.0
    b = Q._abs_table()
    assert np.array_equal(b * 2, np.round(b * 2)) and np.abs(b).max() <= 3.5 and (b * b).sum(-1).max() <= 12.0
    assert np.array_equal(b[:, :7], np.abs(b[:, :7])) and np.array_equal(b[:, 7] < 0, np.abs(b).sum(-1) % 2 == 1)


@pytest.mark.parametrize("name", Q.EXACT_GROUPS)
def test_exact_groups_meet_their_conditions_and_the_rule_is_a_nearest_point_search(name):
    X = Q.search_cases()[name]
    assert X.dtype == np.float32 and X.shape[1] == 8 and 0 < X.shape[0] <= 2048 and Q.scan_is_exact(X)
    stats, rule = Q.search_reference(name)
    print(f"{name}: {X.shape[0]} rows, {int((stats.count > 1).sum())} with ties, up to {stats.count.max()} winners, "
          f"{int(((rule != stats.lowest) & (stats.count > 1)).sum())} tie rows where the rule's code is not the lowest winner")
    assert stats.contains.all()                                  # tie_rule_code(X) lies in exact_winners(X)
    if name in Q.TIE_GROUPS:
        assert (stats.count >= 2).all()
    if name == "dyadic8":
        assert (stats.count >= 2).mean() >= 0.15
    if name == "midpoints":
        assert set(Q.MIDPOINT_KINDS.tolist()) == {0, 1, 2} and len(Q.MIDPOINT_KINDS) == X.shape[0]
    if name == "planes":
        assert stats.count[0] == 2 and stats.count[3] == 2 and stats.count[5] == 16          # 0, 1/2 * 1, e_0
    if name == "outside":
        assert stats.count[192] == 7 and stats.count[-1] == 70 and stats.count[-2] == 70     # 16 e_0, +-4 * 1


def test_winner_stats_is_exact_winners():
    X = Q.search_cases()["holes"][:40]
    rule = Q.tie_rule_code(X)
    win, stats = Q.exact_winners(X), Q.WinnerStats(X, rule)
    assert np.array_equal(win.sum(1), stats.count) and np.array_equal(win.argmax(1), stats.lowest)
    assert np.array_equal(win[np.arange(40), rule], stats.contains)
    r = (np.arange(24).reshape(3, 8) % 5 - 2) / 2.0
    w81 = Q.exact_winners(r, O.e81b_grid())
    assert w81.shape == (3, 256) and w81[np.arange(3), Q.lowest_index_code(r, O.e81b_grid())].all()
    assert Q.exact_winners(np.zeros((1, 8)), O.e81b_grid()).nonzero()[1].tolist() == [56]


def test_tolerance_groups_and_the_bound():
    cases = Q.search_cases()
    assert not Q.nonfinite_rows(cases["huge"]).any() and not Q.nonfinite_rows(cases["tiny"]).any()
    assert Q.nonfinite_rows(cases["nonfinite"]).sum() == 49 and np.abs(cases["huge"]).max() > 1e6
    assert (np.abs(cases["tiny"]) < 1.2e-38).sum() >= 256 and (cases["tiny"] == 0).any()       # subnormals and zeros
    # the float64 nearest point sits inside the bound trivially; a neighbour at squared distance 2 of it does not, as long
    # as the row is not so large that fp32 cannot tell the two apart (the bound then says so)
    X = cases["huge"][:128]
    _, star = O.round_dense(X, O.e8p_full_grid_f64())
    assert (Q.excess_over_nearest(X, star) == 0).all()
    b = Q.score_bound(np.zeros((1, 8)))
    assert 0 < b[0] < 2e-5 and Q.score_bound(np.full((1, 8), 1e6))[0] > 1.0


CASES = [(33, 128, True), (5, 16, False), (1, 8, False)]


@pytest.mark.parametrize("step,s", STEPS)
@pytest.mark.parametrize("m,c,with_p", CASES)
def test_host_models_pass_the_exact_step_check(m, c, with_p, step, s):
    for name, (A, B, M, P) in (("integer_feedback", Q.integer_feedback(m, c, with_p)), ("zero", Q.zero_case(m, c, with_p))):
        hat, idx = Q.run_model(step, A, B, M, P, s)
        rep = Q.check_exact_steps(A, B, M, P, hat, idx, step, s)
        print(f"{name} {step} s={s} ({m}, {c}) P={with_p}: {rep}")
        assert rep.steps == m * (c // 8) and rep.failures == 0
        if name == "zero" and step == "E8P12":
            assert (idx == Q.tie_rule_code(np.zeros((1, 8)))[0]).all()


@pytest.mark.parametrize("step,s", [("E8P12", None), ("E8P12RVQ4B", 0.25), ("E8P12RVQ3B", 0.25)])
def test_host_models_hold_the_fixed_point(step, s):
    W, codes = Q.fixed_point(step, 33, 128, s)
    _, B, M, P = Q.integer_feedback(33, 128, True)
    hat, idx = Q.run_model(step, W, np.zeros_like(W), M, P, s)
    assert np.array_equal(hat, W) and np.array_equal(idx, codes)
    rep = Q.check_exact_steps(W, np.zeros_like(W), M, P, hat, idx, step, s)
    assert rep.failures == 0, str(rep)


def test_fixed_point_pools():
    assert len(Q.stage2_allowed("E8P12RVQ3B", R.DEFAULT_SCALE["E8P12RVQ3B"])) == 241          # 94 % of the E81B entries
    assert len(Q.stage2_allowed("E8P12RVQ4B", R.DEFAULT_SCALE["E8P12RVQ4B"])) == 5176
    for cbid in R.CBIDS:
        W, codes = Q.fixed_point(cbid, 33, 688)
        assert np.array_equal(R.decode_f32(cbid, codes, R.DEFAULT_SCALE[cbid]).reshape(33, 688), W)
        ca, _ = R.split_codes(cbid, codes)
        assert (((W.reshape(33, 86, 8).astype(np.float64) - O.e8p_full_grid_f64()[ca]) ** 2).sum(-1) < 0.49).all()


def test_ill_conditioned_and_saturating_inputs():
    for n in (384, 688):
        H = Q.ill_conditioned_H(n).astype(np.float64)
        ev = np.linalg.eigvalsh(H)
        print(f"ill-conditioned H ({n}): eigenvalues {ev[0]:.4e} .. {ev[-1]:.4e}, condition {ev[-1] / ev[0]:.3e}")
        assert ev[0] > 0 and ev[0] < 0.011 and (ev < 0.011).sum() >= n // 2 and abs(np.diag(H).mean() - 1.01) < 1e-5
        np.linalg.cholesky(H)
    W, _ = Q.saturating(40, 384)
    assert np.abs(W).max() > 1000 and np.isfinite(W).all()


# ---- the checkers against planted faults -------------------------------------------------------------------------------------------

def _search_failures(X, idx, rule, vals=None):
    vals = Q.decode_e8p(idx) if vals is None else vals
    return Q.check_search(X, vals, idx, Q.WinnerStats(X, idx), rule)


def test_checker_catches_the_tied_partner_of_higher_e_par():
    X = Q.search_cases()["midpoints"][:64]
    rule = Q.tie_rule_code(X)
    assert _search_failures(X, rule, rule) == (0, 0, 0)
    win = Q.exact_winners(X)
    win[np.arange(64), rule] = False
    partner = win.argmax(1)                                       # the other of the two winners
    assert win.sum(1).min() == 1
    key = lambda c: (c >> 8) * 2 + (O._popcount8(c & 0xff) & 1)   # noqa: E731   (e, par) in scan order
    later = key(partner) > key(rule)
    assert later.any()
    bad = np.where(later, partner, rule)
    dec, winner, rule_miss = _search_failures(X, bad, rule)
    assert (dec, winner) == (0, 0) and rule_miss == int(later.sum()) >= 1


def test_checker_catches_a_repair_on_the_last_cheapest_column():
    X = Q.search_cases()["repair_ties"]
    rule = Q.search_reference("repair_ties")[1]
    bad = Q.tie_rule_code(X, last_cheapest=True)
    dec, winner, rule_miss = _search_failures(X, bad, rule)
    print(f"last cheapest column: {rule_miss} of {len(X)} rows differ from the rule, {winner} of them no winner at all")
    assert dec == 0 and winner == 0 and rule_miss >= 1            # as near, but not the documented codeword


def test_checker_catches_a_sign_bit():
    X = Q.search_cases()["dyadic8"][:64]
    rule = Q.tie_rule_code(X)
    bad = rule.copy()
    bad[7] ^= 0x10
    dec, winner, rule_miss = _search_failures(X, bad, rule, vals=Q.decode_e8p(rule))
    assert dec >= 1 and rule_miss >= 1
    dec, winner, rule_miss = _search_failures(X, bad, rule)
    assert dec == 0 and winner + rule_miss >= 1


def test_checker_catches_a_near_neighbour_far_outside_the_ball():
    """16 e_0 of `outside` is 13.3 away from its seven nearest codewords.  Moved by eps (w1 - w2) along the difference of two
    of them, w1 alone is nearest and w2 is further by 1e-3: both the membership in exact_winners and the derived score bound
    must refuse w2."""
    x0 = Q.search_cases()["outside"][192:193].astype(np.float64)
    g = O.e8p_full_grid_f64()
    w = Q.exact_winners(x0)[0].nonzero()[0]
    assert len(w) == 7
    w1, w2 = g[w[0]], g[w[1]]
    d0 = np.sqrt(((x0 - w1) ** 2).sum())
    eps = 1e-3 * d0 / ((w1 - w2) ** 2).sum()                      # score(w1) - score(w2) = 2 eps |w1 - w2|^2 = 2 d 1e-3
    X = x0 + eps * (w1 - w2)
    stats = Q.WinnerStats(X, np.array([w[1]]))
    d = np.sqrt(((X - w2) ** 2).sum()), np.sqrt(((X - g[stats.lowest[0]]) ** 2).sum())
    print(f"nearest at {d[1]:.6f}, planted neighbour at {d[0]:.6f}, excess {d[0] - d[1]:.3e}")
    assert stats.count[0] == 1 and 0.5e-3 < d[0] - d[1] < 2e-3
    assert not stats.contains[0]
    assert Q.check_search(X, Q.decode_e8p(w[1:2]), w[1:2], stats, stats.lowest)[1:] == (1, 1)
    assert Q.excess_over_nearest(X, w[1:2])[0] > 2 * Q.score_bound(X)[0]


@pytest.mark.parametrize("step,s", [("E8P12", None), ("E8P12RVQ4B", 0.25), ("E8P12RVQ3B", -1.0)])
def test_step_checker_catches_planted_faults(step, s):
    A, B, M, P = Q.integer_feedback(33, 48, True)
    hat, idx = Q.run_model(step, A, B, M, P, s)
    assert Q.check_exact_steps(A, B, M, P, hat, idx, step, s).failures == 0
    shift = 0 if step == "E8P12" else R.CODE_SHIFT[step]
    bad = idx.copy()
    bad[5, 2] ^= 0x10 << shift                                    # a sign bit of the first stage, hat left as it was
    rep = Q.check_exact_steps(A, B, M, P, hat, bad, step, s)
    assert rep.decode >= 1 and rep.rule >= 1
    if step != "E8P12":
        bad = idx.copy()
        bad[5, 2] ^= 1                                            # the second stage's code
        rep = Q.check_exact_steps(A, B, M, P, hat, bad, step, s)
        assert rep.decode >= 1 and rep.rule2 >= 1 and rep.rule == 0
    # the origin tie of the zero case, resolved to the other winner with hat to match: as near, not the rule's
    Z = Q.zero_case(5, 8, False)
    hat, idx = Q.run_model("E8P12", *Z)
    win = Q.exact_winners(np.zeros((1, 8)))[0].nonzero()[0]
    assert len(win) == 2 and idx[0, 0] in win
    other = int(win[win != idx[0, 0]][0])
    hat2, idx2 = hat.copy(), idx.copy()
    idx2[:, 0] = other
    hat2[:, :8] = Q.decode_e8p(np.array(other))
    rep = Q.check_exact_steps(*Z, hat2, idx2, "E8P12")
    assert rep.decode == 0 and rep.winner == 0 and rep.rule >= 1
