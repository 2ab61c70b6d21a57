"""Float64 checks of the two-stage LDLQ step of the residual codebooks E8P12RVQ4B / E8P12RVQ3B, shared by
tests/test_ldlq_rvq_host.py and tests/test_gpu_ldlq_panel_rvq.py: an oracle codebook (the classes' arithmetic with the float64
brute force as the search of each stage), a torch model of quip_lib::ldlq_panel_rvq, and the per-step consistency checks of
a rounded matrix and its indices.  Inputs, the target and its bound come from tests/ldlq_cases."""
import numpy as np
import torch

from oracle import quip_oracle as O

from tests import ldlq_cases as C

CBIDS = ["E8P12RVQ4B", "E8P12RVQ3B"]
DEFAULT_SCALE = {"E8P12RVQ4B": 1 / 3.45, "E8P12RVQ3B": 1 / 2.04}
CODE_SHIFT = {"E8P12RVQ4B": 16, "E8P12RVQ3B": 8}


def stage2_grid(cbid):
    """float64 table of the second stage: the full E8P12 grid (65 536, 8) or the E81B entries (256, 8)"""
    return O.e8p_full_grid_f64() if cbid == "E8P12RVQ4B" else O.e81b_grid().astype(np.float64)


def split_codes(cbid, idx):
    """(code_a, code_b) of stored indices of any integer dtype (an int32 Qidxs wraps code_a << 16 into the sign bit)"""
    u = np.asarray(idx).astype(np.int64) & 0xffffffff
    sh = CODE_SHIFT[cbid]
    return (u >> sh) & 0xffff, u & ((1 << sh) - 1)


def decode_f32(cbid, idx, s):
    """hat of stored indices by the decoders' stage tables in fp32: fl32(a + fl32(b * fl32(s))), shape idx.shape + (8,)"""
    ca, cb_ = split_codes(cbid, idx)
    a = O.e8p_decode_i8(ca.astype(np.uint16)).astype(np.float32) / np.float32(4)
    if cbid == "E8P12RVQ4B":
        b = O.e8p_decode_i8(cb_.astype(np.uint16)).astype(np.float32) / np.float32(4)
    else:
        b = O.e81b_decode_twice(cb_).astype(np.float32) / np.float32(2)
    bs = (b * np.float32(s)).astype(np.float32)
    return (a + bs).astype(np.float32)


class RvqOracleCodebook:
    """what LDLQ reads of a residual codebook: quantize() is the class's arithmetic in X's dtype
    (codebooks.E8P12RVQ4B_codebook.quantize / E8P12RVQ3B_codebook.quantize) with O.round_dense, the float64 brute force, as
    the search of each stage"""
    codesz, idx_dtype = 8, torch.int32

    def __init__(self, cbid, opt_resid_scale=None):
        assert cbid in CBIDS
        self.id = cbid
        self.opt_resid_scale = DEFAULT_SCALE[cbid] if opt_resid_scale is None else opt_resid_scale

    def _round(self, X, grid):
        vals, ix = O.round_dense(X.detach().cpu().numpy(), grid)
        return torch.from_numpy(vals).to(X.dtype), torch.from_numpy(ix)

    def quantize(self, X, return_idx=True):
        init_vals, init_idxs = self._round(X, O.e8p_full_grid_f64())
        resid_vals, resid_idxs = self._round((X - init_vals) / self.opt_resid_scale, stage2_grid(self.id))
        final = init_vals + resid_vals * self.opt_resid_scale
        return (final, (init_idxs << CODE_SHIFT[self.id]) + resid_idxs) if return_idx else final


def panel_model_rvq(cb):
    """panel_fn(A, B, M, P) for quant.LDLQ_panels: the recursion of quip_lib::ldlq_panel_rvq in torch, in the operands' dtype,
    with cb.quantize (an RvqOracleCodebook) as the step"""
    def panel_fn(A, B, M, P):
        m, c = A.shape
        hat, E = torch.zeros_like(A), torch.zeros_like(A)
        idx = torch.zeros(m, c // 8, dtype=torch.int64)
        for k in range(c // 8 - 1, -1, -1):
            lo, hi = 8 * k, 8 * k + 8
            t = B[:, lo:hi] + E[:, hi:] @ M[hi:, lo:hi]
            if P is not None:
                t = t @ P[k]
            hat[:, lo:hi], idx[:, k] = cb.quantize(A[:, lo:hi] + t)
            E[:, lo:hi] = A[:, lo:hi] - hat[:, lo:hi]
        return hat, idx
    return panel_fn


class StepReport:
    """counts over all steps checked: over1 / over2 = steps whose stage-1 / stage-2 point is further than the bound allows,
    hat_wrong = steps where hat is not fl32(a + fl32(b s)) of its own codes, worst1 / worst2 = largest excess over the
    nearest point"""
    def __init__(self):
        self.over1 = self.over2 = self.hat_wrong = self.steps = 0
        self.worst1 = self.worst2 = 0.0

    @property
    def over(self):
        return self.over1 + self.over2 + self.hat_wrong

    def __str__(self):
        return (f"{self.over1} (stage 1) + {self.over2} (stage 2) of {self.steps} steps over the bound, {self.hat_wrong} with "
                f"another hat than their codes decode to; largest excess {self.worst1:.3e} / {self.worst2:.3e}")


def _check_two_stages(rep, cbid, s, t, eps, hat_k, idx_k):
    """one group of every row: t (m, 8) float64 target, eps (m,) its fp32 accumulation bound, hat_k (m, 8) fp32, idx_k (m,)"""
    s32 = float(np.float32(s))
    ca, cb_ = split_codes(cbid, idx_k)
    g1, g2 = O.e8p_full_grid_f64(), stage2_grid(cbid)
    a, b = g1[ca], g2[cb_]
    want = (a.astype(np.float32) + (b.astype(np.float32) * np.float32(s)).astype(np.float32)).astype(np.float32)
    rep.hat_wrong += int((want != np.asarray(hat_k, np.float32)).any(axis=1).sum())
    astar, _ = O.round_dense(t, g1)
    d, dstar = np.linalg.norm(t - a, axis=1), np.linalg.norm(t - astar, axis=1)
    rep.over1 += int((d > dstar + 2.0 * eps).sum())
    rep.worst1 = max(rep.worst1, float((d - dstar).max()))
    # the residual the second stage rounds, formed from the first stage's own point; its fp32 value carries the target's
    # error divided by |s| plus three roundings (the subtraction, the division, one conversion), each u ||r||
    r = (t - a) / s32
    bstar, _ = O.round_dense(r, g2)
    d, dstar = np.linalg.norm(r - b, axis=1), np.linalg.norm(r - bstar, axis=1)
    eps2 = eps / abs(s32) + 3.0 * C.U32 * np.linalg.norm(r, axis=1)
    rep.over2 += int((d > dstar + 2.0 * eps2).sum())
    rep.worst2 = max(rep.worst2, float((d - dstar).max()))
    rep.steps += t.shape[0]


def check_rvq_steps(cbid, W, Lb, hat, idx, s=None):
    """Every step of an LDLQ pass of a residual codebook against float64.  Target and bound of group k exactly as in
    ldlq_cases.check_ldlq_steps (from W, the float64 block-LDL factor Lb and the GIVEN hat right of k).  The stored index
    splits into the two stage codes, decoded to a (O.e8p_full_grid_f64) and b (the same grid, or O.e81b_grid); required:
        hat_k == fl32(a + fl32(b s32))                                    exactly,
        ||t - a|| <= ||t - a*|| + 2 eps,                                   a* the float64 nearest first-stage point of t,
        ||r - b|| <= ||r - b*|| + 2 (eps / |s| + 3 u ||r||),   r = (t - a) / s32 in float64, b* its nearest second-stage point.
    Returns a StepReport."""
    s = DEFAULT_SCALE[cbid] if s is None else s
    W, hat64 = np.asarray(W, np.float64), np.asarray(hat, np.float64)
    m, n = W.shape
    E, absL = W - hat64, np.abs(Lb)
    rep = StepReport()
    for k in range(n // 8 - 1, -1, -1):
        lo, hi = 8 * k, 8 * k + 8
        t = W[:, lo:hi] + E[:, hi:] @ Lb[hi:, lo:hi]
        eps = (n - hi + 2) * C.U32 * np.linalg.norm(np.abs(W[:, lo:hi]) + np.abs(E[:, hi:]) @ absL[hi:, lo:hi], axis=1)
        _check_two_stages(rep, cbid, s, t, eps, np.asarray(hat)[:, lo:hi], np.asarray(idx)[:, k])
    return rep


def check_rvq_tune_steps(cbid, W, H, hat_before, hat_after, idx_after, s=None):
    """The same two stages for one tune sweep, on the target and bound of ldlq_cases.check_tune_steps"""
    s = DEFAULT_SCALE[cbid] if s is None else s
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    hb, ha = np.asarray(hat_before, np.float64), np.asarray(hat_after, np.float64)
    m, n = W.shape
    rep = StepReport()
    for k in range(n // 8 - 1, -1, -1):
        lo, hi = 8 * k, 8 * k + 8
        mixed = np.concatenate([hb[:, :hi], ha[:, hi:]], axis=1)
        D = W - mixed
        Pk = np.linalg.inv(H[lo:hi, lo:hi])
        t = hb[:, lo:hi] + D @ H[:, lo:hi] @ Pk
        eps = (n + 10) * C.U32 * np.linalg.norm(np.abs(hb[:, lo:hi]) + np.abs(D) @ np.abs(H[:, lo:hi]) @ np.abs(Pk), axis=1)
        _check_two_stages(rep, cbid, s, t, eps, np.asarray(hat_after)[:, lo:hi], np.asarray(idx_after)[:, k])
    return rep
