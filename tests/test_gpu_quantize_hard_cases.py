"""The quantiser (csrc/quantize.hip) on exact ties, deep holes, points far outside the ball and saturating panels
(tests/quantize_hard_cases.py).  On the exact inputs no fp32 rounding takes part in the scan, so every comparison is an
equality: the values are the decode of the code, the code is an exactly nearest codeword of the float64 brute force, and it is
the one the documented tie rule names -- for e8p_quantize on eight lanes and on one, and for every group of the three panel
templates.  The only tolerances are the derived score bound of the tolerance groups and the fp32 accumulation bound of the
existing step checks."""
import numpy as np
import pytest
import torch

from oracle import quip_oracle as O
from quip_for_all_amd import quant

from tests import ldlq_cases as C
from tests import ldlq_rvq_cases as R
from tests import quantize_hard_cases as Q

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
STEPS = ["E8P12", "E8P12RVQ4B", "E8P12RVQ3B"]
_SEARCHED, _CODEBOOKS = {}, {}


def _say(line):
    print(f"[quantize_hard_cases] {line}")


def _cb(cbid, **kw):
    import quip_for_all_amd as QA
    key = (cbid, tuple(sorted(kw.items())))
    if key not in _CODEBOOKS:
        _CODEBOOKS[key] = QA.codebook.codebook_id[cbid](inference=False, **kw).to(DEV)
    return _CODEBOOKS[key]


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _e8p(X):
    """e8p_quantize of a numpy (N, 8) fp32 array -> (vals, idx) numpy"""
    vals, idx = torch.ops.quip_lib.e8p_quantize(_dev(X), _cb("E8P12").grid_packed_abs)
    return vals.cpu().numpy(), idx.cpu().numpy()


def _searched(name):
    if name not in _SEARCHED:
        X = Q.search_cases()[name]
        assert X.shape[0] < 65536                                  # the eight-lane instantiation
        _SEARCHED[name] = _e8p(X)
    return _SEARCHED[name]


def _panel(step, A, B, M, P, s=None):
    """one direct call of the step's op on numpy operands -> (hat, idx) numpy"""
    A, B, M, P = _dev(A), _dev(B), _dev(M), _dev(P)
    if step == "E8P12":
        hat, idx = torch.ops.quip_lib.ldlq_panel(A, B, M, P, _cb(step).grid_packed_abs)
    else:
        cb = _cb(step)
        resid = cb.e81b_grid.to(torch.float32).contiguous() if step == "E8P12RVQ3B" else None
        hat, idx = torch.ops.quip_lib.ldlq_panel_rvq(A, B, M, P, cb.grid_packed_abs, resid, float(s))
    return hat.cpu().numpy(), idx.cpu().numpy()


# ---- e8p_quantize ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", Q.EXACT_GROUPS)
def test_exact_groups_on_eight_lanes(name):
    X = Q.search_cases()[name]
    vals, idx = _searched(name)
    ref, rule = Q.search_reference(name)
    dec, winner, rule_miss = Q.check_search(X, vals, idx, Q.WinnerStats(X, idx), rule)
    ties = ref.count > 1
    _say(f"search {name}: rows {X.shape[0]}, with ties {int(ties.sum())}, largest winner count {ref.count.max()}, mismatches "
         f"{dec} (decode) {winner} (no exact winner) {rule_miss} (not the tie rule's code)")
    assert dec == 0                                             # vals == decode(idx)
    assert winner == 0                                          # idx in exact_winners
    assert rule_miss == 0                                       # idx == tie_rule_code


def test_one_lane_repeats_the_eight_lane_result():
    cases = Q.search_cases()
    X = np.concatenate([cases[k] for k in Q.EXACT_GROUPS + Q.TOLERANCE_GROUPS])
    reps = -(-65536 // X.shape[0])
    assert X.shape[0] < 65536 <= reps * X.shape[0]
    cb = _cb("E8P12")
    v8, i8 = torch.ops.quip_lib.e8p_quantize(_dev(X), cb.grid_packed_abs)
    v1, i1 = torch.ops.quip_lib.e8p_quantize(_dev(np.tile(X, (reps, 1))), cb.grid_packed_abs)
    assert torch.isfinite(v8).all() and torch.isfinite(v1).all()
    assert torch.equal(i1.reshape(reps, -1), i8.expand(reps, -1))
    assert torch.equal(v1.reshape(reps, -1, 8), v8.expand(reps, -1, 8))
    _say(f"one lane: {reps} x {X.shape[0]} vectors equal the eight-lane result bit for bit")


@pytest.mark.parametrize("name", ["huge", "tiny"])
def test_tolerance_groups_stay_inside_the_derived_bound(name):
    X = Q.search_cases()[name]
    vals, idx = _e8p(X)
    assert np.array_equal(vals, Q.decode_e8p(idx))
    excess, bound = Q.excess_over_nearest(X, idx), Q.score_bound(X)
    _say(f"search {name}: rows {X.shape[0]}, worst excess over the nearest point {excess.max():.3e} (squared distance), worst "
         f"excess / (2 bound) {np.max(excess / (2 * bound)):.3e}, rows off the float64 arg max {int((excess > 0).sum())}")
    assert (excess <= 2.0 * bound).all()


def test_nonfinite_rows_get_codes_and_leave_the_others_alone():
    X = Q.search_cases()["nonfinite"]
    bad = Q.nonfinite_rows(X)
    vals, idx = _e8p(X)
    assert ((idx >= 0) & (idx < 65536)).all() and np.array_equal(vals, Q.decode_e8p(idx))
    v_good, i_good = _e8p(X[~bad])
    assert np.array_equal(idx[~bad], i_good) and np.array_equal(vals[~bad], v_good)
    _say(f"search nonfinite: {int(bad.sum())} of {X.shape[0]} rows non-finite, all codes in range, the other rows unchanged")


def test_report_share_off_the_lowest_code():
    """The reference's GEMM arg max takes the lowest code among equal scores; the kernel promises its own order.  Reported, not
    asserted: a checkpoint quantised here can differ from the reference's on exactly these rows."""
    ties = differ = 0
    for name in Q.EXACT_GROUPS:
        ref, _ = Q.search_reference(name)
        _, idx = _searched(name)
        t = ref.count > 1
        ties += int(t.sum())
        differ += int((idx[t] != ref.lowest[t]).sum())
    _say(f"reference order: {differ} of {ties} tie rows ({differ / ties:.1%}) take another code than the lowest-code winner")
    assert ties > 0


# ---- direct panel calls on exact operands ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("with_p", [False, True])
@pytest.mark.parametrize("c", Q.PANEL_C)
@pytest.mark.parametrize("m", Q.PANEL_M)
@pytest.mark.parametrize("step,s", [("E8P12", None)] + [(cbid, s) for cbid in R.CBIDS for s in Q.EXACT_SCALES])
def test_exact_panels(step, s, m, c, with_p):
    for name, ops in (("integer_feedback", Q.integer_feedback(m, c, with_p)), ("zero", Q.zero_case(m, c, with_p))):
        hat, idx = _panel(step, *ops, s)
        rep = Q.check_exact_steps(*ops, hat, idx, step, s)
        _say(f"panel {name} {step} s={s} ({m}, {c}) P={with_p}: {rep}")
        assert rep.steps == m * (c // 8) and rep.failures == 0, str(rep)


def test_three_templates_and_e8p_quantize_choose_the_same_first_stage():
    """the exact search inputs as panel targets with M = 0: 16 groups per row"""
    cases = Q.search_cases()
    X = np.concatenate([cases[k] for k in Q.EXACT_GROUPS])
    m = X.shape[0] // 16
    X = X[:16 * m]
    A = X.reshape(m, 128)
    _, want = _e8p(X)
    want = want.reshape(m, 16)
    Z, M0 = np.zeros_like(A), np.zeros((128, 128), np.float32)
    _, idx = _panel("E8P12", A, Z, M0, None)
    assert np.array_equal(idx, want)
    for step in R.CBIDS:
        for s in Q.EXACT_SCALES:
            hat, idx = _panel(step, A, Z, M0, None, s)
            assert np.array_equal(R.split_codes(step, idx)[0], want), (step, s)
            assert np.array_equal(hat, R.decode_f32(step, idx, s).reshape(m, 128))
    _say(f"first stage: {16 * m} exact targets get the same code from e8p_quantize and the three panel templates")


# ---- fixed points: W made of codewords ----------------------------------------------------------------------------------------

def _routes(W, H, cb, iters):
    L = np.linalg.cholesky(H.astype(np.float64)).astype(np.float32)
    for run in (quant.LDLQ_panels, quant.LDLQ_stepwise):
        hat, Qi = run(_dev(W).clone(), _dev(H).clone(), _dev(L).clone(), cb, iters)
        yield run.__name__, hat.cpu().numpy(), Qi.cpu().numpy()


@pytest.mark.parametrize("m,n", Q.ILL_SHAPES)
@pytest.mark.parametrize("step,s", [("E8P12", None), ("E8P12RVQ4B", 0.25), ("E8P12RVQ4B", None), ("E8P12RVQ3B", 0.25),
                                    ("E8P12RVQ3B", None)])
def test_codeword_matrices_are_fixed_points(step, s, m, n):
    """whatever H: the feedback is identically zero, hat == W bit for bit and idx are the planted codes, on both routes, main
    pass and tune sweep.  s = None: the codebook's default scale."""
    W, codes = Q.fixed_point(step, m, n, s)
    H = Q.ill_conditioned_H(n)
    cb = _cb(step) if s is None else _cb(step, opt_resid_scale=s)
    mask = 0xffff if step == "E8P12" else 0xffffffff
    for iters in (0, 1):
        for route, hat, Qi in _routes(W, H, cb, iters):
            assert np.array_equal(hat, W), (route, iters)
            assert np.array_equal(Qi.astype(np.int64) & mask, codes), (route, iters)
    _say(f"fixed point {step} s={s} ({m}, {n}): hat == W and the planted codes on both routes, iters 0 and 1")


# ---- ill-conditioned H and saturating W: the bounded step checks ---------------------------------------------------------------------

_HARD = {}


def _hard(step, case, m, n):
    """LDLQ_panels with 0 and 1 tune sweeps, once per case: (W, H, L64, hat0, Q0, hat1, Q1) as numpy"""
    key = (step, case, m, n)
    if key not in _HARD:
        W, H = getattr(Q, case)(m, n)
        L64 = C.chol64(H)
        Wt, Ht, Lt = _dev(W), _dev(H), _dev(L64.astype(np.float32))
        out = [W, H, L64]
        for iters in (0, 1):
            out += [t.cpu().numpy() for t in quant.LDLQ_panels(Wt.clone(), Ht.clone(), Lt.clone(), _cb(step), iters)]
        _HARD[key] = tuple(out)
    return _HARD[key]


def _decoded(step, Qi, m, n):
    if step == "E8P12":
        return Q.decode_e8p(Qi).reshape(m, n)
    return R.decode_f32(step, Qi, R.DEFAULT_SCALE[step]).reshape(m, n)


@pytest.mark.parametrize("m,n", Q.ILL_SHAPES)
@pytest.mark.parametrize("case", ["ill_conditioned", "saturating"])
@pytest.mark.parametrize("step", STEPS)
def test_hard_panels_main_pass(step, case, m, n):
    """ldlq_cases.check_ldlq_steps / ldlq_rvq_cases.check_rvq_steps as they are, called as tests/test_gpu_ldlq_panel*.py call
    them; the proxy losses of the two routes and of the float64 oracle are written out, not asserted"""
    W, H, L64, hat0, Q0, _, _ = _hard(step, case, m, n)
    Lb = O.block_ldl(L64, 8)
    if step == "E8P12":
        over, steps, worst = C.check_ldlq_steps(W, Lb, hat0)
    else:
        rep = R.check_rvq_steps(step, W, Lb, hat0, Q0)
        over, steps, worst = rep.over, rep.steps, max(rep.worst1, rep.worst2)
    Wt, Ht, Lt = _dev(W), _dev(H), _dev(L64.astype(np.float32))
    stepwise, _ = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), _cb(step), 0)
    oracle, _ = O.ldlq(W, H, step, 0)
    _say(f"panel {case} {step} ({m}, {n}) main pass: steps {steps}, over {over}, worst excess {worst:.3e}, proxy loss panels "
         f"{C.proxy_loss(W, hat0, H):.6e} stepwise {C.proxy_loss(W, stepwise.cpu().numpy(), H):.6e} float64 oracle "
         f"{C.proxy_loss(W, oracle, H):.6e}")
    assert steps == m * (n // 8)
    assert over == 0
    assert np.array_equal(hat0, _decoded(step, Q0, m, n))


@pytest.mark.parametrize("m,n", Q.ILL_SHAPES)
@pytest.mark.parametrize("case", ["ill_conditioned", "saturating"])
@pytest.mark.parametrize("step", STEPS)
def test_hard_panels_tune_sweep(step, case, m, n):
    W, H, _, hat0, _, hat1, Q1 = _hard(step, case, m, n)
    if step == "E8P12":
        over, steps, worst = C.check_tune_steps(W, H, hat0, hat1)
    else:
        rep = R.check_rvq_tune_steps(step, W, H, hat0, hat1, Q1)
        over, steps, worst = rep.over, rep.steps, max(rep.worst1, rep.worst2)
    _say(f"panel {case} {step} ({m}, {n}) tune sweep: steps {steps}, over {over}, worst excess {worst:.3e}, proxy loss "
         f"{C.proxy_loss(W, hat0, H):.6e} -> {C.proxy_loss(W, hat1, H):.6e}")
    assert steps == m * (n // 8)
    assert over == 0
    assert np.array_equal(hat1, _decoded(step, Q1, m, n))


# ---- poisoned rows ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m,c", [(33, 48), (40, 128)])
@pytest.mark.parametrize("step", STEPS)
def test_poisoned_rows_stay_in_their_rows(step, m, c):
    """one row all NaN (the last one: at m = 33 the 31 idle row slots of the second workgroup replicate it), one with +inf, one
    with 3e38: every other row is, bit for bit, what the launch without them gives"""
    A, B, M, P, bad = Q.poisoned(m, c)
    s = None if step == "E8P12" else R.DEFAULT_SCALE[step]
    good = np.setdiff1d(np.arange(m), bad)
    hat, idx = _panel(step, A, B, M, P, s)
    hat_g, idx_g = _panel(step, A[good], B[good], M, P, s)
    assert np.array_equal(idx[good], idx_g) and np.array_equal(hat[good], hat_g)
    assert np.isfinite(hat_g).all()
    top = {"E8P12": 1 << 16, "E8P12RVQ4B": 1 << 32, "E8P12RVQ3B": 1 << 24}[step]
    assert ((idx >= 0) & (idx < top)).all()
    dec = Q.decode_e8p(idx) if step == "E8P12" else R.decode_f32(step, idx, s)
    fin = np.isfinite(hat)
    assert np.array_equal(hat[fin], dec.reshape(m, c)[fin])
    _say(f"panel poisoned {step} ({m}, {c}): {len(good)} ordinary rows unchanged, {int((~fin).sum())} non-finite hat entries in "
         f"rows {sorted(set(np.nonzero(~fin)[0].tolist()))}")
