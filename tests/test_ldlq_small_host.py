"""Host side of the fused LDLQ panels for D4 / HI (no GPU): the C entry's header, the QUIP_LDLQ_FUSED_SMALL switch in
ldlq_route, and LDLQ_panels_small against the stepwise loop in float64."""
import os
import re

import pytest
import torch

from oracle import quip_oracle as O
from quip_for_all_amd import capi, quant

from tests import ldlq_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SmallOracleCodebook:
    """tests/ldlq_cases.OracleCodebook for the narrow codebooks: what LDLQ reads, the float64 brute force as the search"""
    def __init__(self, cbid):
        self.id, self.codesz = cbid, O.code_size(cbid)
        self.idx_dtype = torch.uint8 if cbid == "D4" else torch.int32

    def quantize(self, X, return_idx=True):
        vals, ix = O.quantize(self.id, X.detach().cpu().numpy())
        vals = torch.from_numpy(vals).to(X.dtype)
        return (vals, torch.from_numpy(ix)) if return_idx else vals


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "quip_mi355.h")).read()
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 24
    decl = re.search(r"int quip_ldlq_panel_small_f32\(([^;]*)\);", src)
    assert "const void* grid, int32_t codesz, void* hat, void* idx, quip_stream_t stream" in " ".join(decl.group(1).split())
    assert capi.lib().quip_abi_version() >= 24 and "quip_ldlq_panel_small_f32" in capi.SIGNATURES


class _OnGpu:
    """what ldlq_route reads of a tensor, claiming to be an fp32 GPU tensor"""
    is_cuda, dtype = True, torch.float32


@pytest.mark.parametrize("cbid", ["D4", "HI"])
def test_route(cbid, monkeypatch):
    cb = SmallOracleCodebook(cbid)
    want = {(None, None): "stepwise", (None, "0"): "stepwise", (None, "1"): "panels", ("0", "1"): "stepwise",
            ("1", "1"): "panels", ("1", None): "stepwise"}
    for (fused, small), route in want.items():
        monkeypatch.setattr(quant, "_LDLQ_FUSED", None)
        monkeypatch.setattr(quant, "_LDLQ_FUSED_SMALL", None)
        for name, value in (("QUIP_LDLQ_FUSED", fused), ("QUIP_LDLQ_FUSED_SMALL", small)):
            monkeypatch.delenv(name, raising=False) if value is None else monkeypatch.setenv(name, value)
        assert quant.ldlq_route(_OnGpu(), cb) == route, (fused, small)
        assert quant.ldlq_route(torch.zeros(4, 16), cb) == "stepwise"            # the CPU
        assert quant.ldlq_route(_OnGpu(), C.OracleCodebook()) == ("stepwise" if fused == "0" else "panels")
    with pytest.raises(ValueError):
        quant.small_panel_launch(C.OracleCodebook(), torch.device("cpu"))


def _panel_model(cb):
    """panel_fn(A, B, M, P): the recursion of quip_lib::ldlq_panel_small in torch, in the operands' dtype"""
    def run(A, B, M, P):
        b = cb.codesz
        hat, idx = torch.zeros_like(A), torch.zeros(A.shape[0], A.shape[1] // b, dtype=torch.int64)
        for k in range(A.shape[1] // b - 1, -1, -1):
            lo, hi = b * k, b * k + b
            t = B[:, lo:hi] + (A[:, hi:] - hat[:, hi:]) @ M[hi:, lo:hi]
            hat[:, lo:hi], idx[:, k] = cb.quantize(A[:, lo:hi] + (t if P is None else t @ P[k]))
        return hat, idx
    return run


@pytest.mark.parametrize("iters", [0, 1])
@pytest.mark.parametrize("cbid", ["D4", "HI"])
def test_panel_recursion_reproduces_stepwise_ldlq(cbid, iters):
    """LDLQ_panels_small driven by the float64 model against LDLQ_stepwise, both with the brute force as the search: equal
    indices, or, where a tie resolved differently, equal distance to the stepwise target at the first group that differs"""
    W, H = (torch.from_numpy(a).double() for a in C.make_case(40, 384))
    L, cb, b = torch.linalg.cholesky(H), SmallOracleCodebook(cbid), O.code_size(cbid)
    hat_s, q_s = quant.LDLQ_stepwise(W.clone(), H.clone(), L.clone(), cb, iters)
    hat_p, q_p = quant.LDLQ_panels_small(W.clone(), H.clone(), L.clone(), cb, iters, panel_fn=_panel_model(cb))
    assert q_s.dtype == q_p.dtype == cb.idx_dtype and tuple(q_p.shape) == (40, 384 // b)
    for row in (q_s != q_p).any(dim=1).nonzero().flatten().tolist():
        col = int((q_s[row] != q_p[row]).nonzero().max())                     # the first group rounded (rightmost) that differs
        assert iters == 0, "ties are settled in the main pass"
        lo, hi = b * col, b * col + b
        t = W[row, lo:hi] + (W[row, hi:] - hat_s[row, hi:]) @ quant.block_LDL(L.clone(), b)[hi:, lo:hi]
        assert abs((t - hat_s[row, lo:hi]).norm().item() - (t - hat_p[row, lo:hi]).norm().item()) <= 1e-12, (row, col)
