"""Inputs and float64 checks shared by the LDLQ panel tests (host: tests/test_quantize_model_host.py, GPU:
tests/test_gpu_ldlq_panel.py): small (W, H) cases, a pure-torch model of the recursion of ldlq_panel_kernel with the
brute-force oracle as the search, and the per-step consistency check of a rounded matrix against float64."""
import numpy as np
import torch

from oracle import quip_oracle as O

# (m, n): three panels and m no multiple of a row tile | one short panel | leftmost panel of 48 columns | one group
SHAPES = [(40, 384), (24, 64), (33, 688), (5, 8)]
U32 = 2.0 ** -24          # unit roundoff of fp32


def make_case(m, n, seed=0):
    """W (m, n) fp32 at the codebook's scale with some rows three times larger and one row all zeros; H (n, n) fp32 from
    correlated random activations, mean diagonal 1, plus 0.01 I"""
    rng = np.random.default_rng(1000 * m + n + seed)
    mix = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    mix[:, : max(1, n // 8)] += 0.5 * rng.standard_normal((n, 1))         # a few directions shared by every feature
    X = rng.standard_normal((4 * n + 64, n)) @ mix
    H = X.T @ X / X.shape[0]
    H = H / np.diag(H).mean() + 0.01 * np.eye(n)
    W = rng.standard_normal((m, n)) * 0.97
    W[1::7] *= 3.0
    W[min(3, m - 1)] = 0.0
    return W.astype(np.float32), H.astype(np.float32)


def chol64(H):
    return np.linalg.cholesky(np.asarray(H, np.float64))


def proxy_loss(W, hat, H):
    D = np.asarray(W, np.float64) - np.asarray(hat, np.float64)
    return float(np.trace(D @ np.asarray(H, np.float64) @ D.T))


def panel_model(A, B, M, P, quantize=None):
    """the recursion of quip_lib::ldlq_panel in torch, in the operands' dtype, with oracle.quantize as the search (or
    quantize(X numpy) -> (vals, idx) in its place)"""
    if quantize is None:
        quantize = lambda X: O.quantize("E8P12", X)      # noqa: E731
    m, c = A.shape
    hat, E = torch.zeros_like(A), torch.zeros_like(A)
    idx = torch.zeros(m, c // 8, dtype=torch.int64)
    for k in range(c // 8 - 1, -1, -1):
        lo, hi = 8 * k, 8 * k + 8
        t = B[:, lo:hi] + E[:, hi:] @ M[hi:, lo:hi]
        if P is not None:
            t = t @ P[k]
        vals, ix = quantize((A[:, lo:hi] + t).numpy())
        hat[:, lo:hi] = torch.from_numpy(vals).to(A.dtype)
        idx[:, k] = torch.from_numpy(ix)
        E[:, lo:hi] = A[:, lo:hi] - hat[:, lo:hi]
    return hat, idx


class OracleCodebook:
    """what LDLQ reads of a codebook, with the float64 brute force behind quantize()"""
    id, codesz, idx_dtype = "E8P12", 8, torch.int64

    def quantize(self, X, return_idx=True):
        vals, ix = O.quantize("E8P12", X.detach().cpu().numpy())
        vals = torch.from_numpy(vals).to(X.dtype)
        return (vals, torch.from_numpy(ix)) if return_idx else vals


def _nearest_check(t, g, eps):
    """rows where ||t - g|| > ||t - g*|| + 2 eps, g* the float64 nearest codeword of t"""
    gstar, _ = O.quantize("E8P12", t)
    d, dstar = np.linalg.norm(t - g, axis=1), np.linalg.norm(t - gstar, axis=1)
    return d > dstar + 2.0 * eps, d - dstar


def check_ldlq_steps(W, Lb, hat):
    """Every step of an LDLQ pass against float64: for each group k the target recomputed from W, the block-LDL factor
    Lb (float64) and the GIVEN hat right of k; the given hat_k must be a nearest codeword of it up to the fp32
    accumulation bound of that target,
        eps_k = (terms + 2) u || |W_k| + |E| |Lb_{>k,k}| ||,   terms = columns right of k, u = 2^-24
    (a dot product of `terms` terms plus the two additions, each with relative error u, first order).
    Returns (steps over the bound, steps, largest excess over ||t - g*||)."""
    W, hat = np.asarray(W, np.float64), np.asarray(hat, np.float64)
    m, n = W.shape
    E, absL = W - hat, np.abs(Lb)
    over, worst = 0, 0.0
    for k in range(n // 8 - 1, -1, -1):
        lo, hi = 8 * k, 8 * k + 8
        t = W[:, lo:hi] + E[:, hi:] @ Lb[hi:, lo:hi]
        eps = (n - hi + 2) * U32 * np.linalg.norm(np.abs(W[:, lo:hi]) + np.abs(E[:, hi:]) @ absL[hi:, lo:hi], axis=1)
        bad, excess = _nearest_check(t, hat[:, lo:hi], eps)
        over += int(bad.sum())
        worst = max(worst, float(excess.max()))
    return over, m * (n // 8), worst


def check_tune_steps(W, H, hat_before, hat_after):
    """The same for one tune sweep: the target of group k is recomputed in float64 from the pre-sweep hat for j <= k and
    the post-sweep hat for j > k,
        t_k = hat_before_k + (W - hat_mixed) H[:, k] inv(H_kk),
    with the accumulation bound eps_k = (n + 8 + 2) u || |hat_before_k| + (|W - hat_mixed| |H[:, k]|) |inv(H_kk)| ||."""
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    hb, ha = np.asarray(hat_before, np.float64), np.asarray(hat_after, np.float64)
    m, n = W.shape
    over, worst = 0, 0.0
    for k in range(n // 8 - 1, -1, -1):
        lo, hi = 8 * k, 8 * k + 8
        mixed = np.concatenate([hb[:, :hi], ha[:, hi:]], axis=1)
        D = W - mixed
        Pk = np.linalg.inv(H[lo:hi, lo:hi])
        t = hb[:, lo:hi] + D @ H[:, lo:hi] @ Pk
        eps = (n + 10) * U32 * np.linalg.norm(np.abs(hb[:, lo:hi]) + np.abs(D) @ np.abs(H[:, lo:hi]) @ np.abs(Pk), axis=1)
        bad, excess = _nearest_check(t, ha[:, lo:hi], eps)
        over += int(bad.sum())
        worst = max(worst, float(excess.max()))
    return over, m * (n // 8), worst
