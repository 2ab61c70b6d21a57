"""Host side of the fused LDLQ panels for E8P12RVQ4B / E8P12RVQ3B (no GPU): the C entry's header and refusals, the op's fake,
the QUIP_LDLQ_FUSED_RVQ switch and the route, the panel recursion against the stepwise loop in float64, and the float64 step
checks of tests/ldlq_rvq_cases.py met by the repository's own fp32 stepwise loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from quip_for_all_amd import quant

from tests import ldlq_cases as C
from tests import ldlq_rvq_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry():
    src = open(os.path.join(ROOT, "include", "quip_mi355.h")).read()
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 23
    decl = re.search(r"int quip_ldlq_panel_rvq_f32\(([^;]*)\);", src)
    assert decl is not None
    args = " ".join(decl.group(1).split())
    assert "const void* resid_grid, float resid_scale" in args and args.endswith("quip_stream_t stream")
    from quip_for_all_amd import capi
    assert capi.lib().quip_abi_version() >= 23 and "quip_ldlq_panel_rvq_f32" in capi.SIGNATURES


# ---- the C entry: every refusal comes before a launch -------------------------------------------------------------------
def test_c_entry_checks_its_arguments():
    from quip_for_all_amd import capi
    L = capi.lib()
    buf = (ctypes.c_char * 16384)()
    a = (ctypes.addressof(buf) + 63) & ~63
    f = L.quip_ldlq_panel_rvq_f32
    s = 1 / 3.45
    for grid2 in (None, a):
        assert f(a, a, a, None, 0, 128, a, grid2, s, a, a, None) == 0            # m == 0: ok, no launch
        assert f(a, a, a, None, -1, 128, a, grid2, s, a, a, None) == -2
        assert f(a, a, a, None, 4, 12, a, grid2, s, a, a, None) == -2            # c % 8
        assert f(a, a, a, None, 4, 0, a, grid2, s, a, a, None) == -2
        assert f(a, a, a, None, 4, 136, a, grid2, s, a, a, None) == -5           # c > 128
        for bad in (0.0, -0.0, float("inf"), float("-inf"), float("nan"), 1e39):   # 1e39 is inf as fp32
            assert f(a, a, a, None, 4, 8, a, grid2, bad, a, a, None) == -2, bad
        for hole in range(3):
            args = [a, a, a]
            args[hole] = None
            assert f(*args, None, 4, 8, a, grid2, s, a, a, None) == -1
        assert f(a, a, a, None, 4, 8, None, grid2, s, a, a, None) == -1
        assert f(a, a, a, None, 4, 8, a, grid2, s, None, a, None) == -1
        assert f(a, a, a, None, 4, 8, a, grid2, s, a, None, None) == -1
        assert f(a + 4, a, a, None, 4, 8, a, grid2, s, a, a, None) == -3
        assert f(a, a, a, a + 4, 4, 8, a, grid2, s, a, a, None) == -3
        assert f(a, a, a, None, 4, 8, a, grid2, s, a + 4, a, None) == -3
        assert f(a, a, a, None, 4, 8, a, grid2, s, a, a + 4, None) == -3         # idx: 8-byte aligned
    assert f(a, a, a, None, 4, 8, a, a + 4, s, a, a, None) == -3                 # resid_grid: 16-byte aligned
    assert f(a, a, a, None, 4, 8, a, a + 8, -1.0, a, a, None) == -3              # (a negative scale is a value, not a refusal)


def test_op_fake_shapes():
    t = lambda *s, dtype=torch.float32: torch.empty(*s, dtype=dtype, device="meta")   # noqa: E731
    op = torch.ops.quip_lib.ldlq_panel_rvq
    hat, idx = op(t(40, 48), t(40, 48), t(48, 48), None, t(256, dtype=torch.int64), None, 1 / 3.45)
    assert (tuple(hat.shape), hat.dtype, tuple(idx.shape), idx.dtype) == ((40, 48), torch.float32, (40, 6), torch.int64)
    hat, idx = op(t(3, 8), t(3, 8), t(8, 8), t(1, 8, 8), t(256, dtype=torch.int64), t(256, 8), 1 / 2.04)
    assert (tuple(hat.shape), tuple(idx.shape), idx.dtype) == ((3, 8), (3, 1), torch.int64)


# ---- the switch and the route --------------------------------------------------------------------------------------------
def test_rvq_switch_parses(monkeypatch):
    assert quant.parse_ldlq_fused(None, default=False) is False and quant.parse_ldlq_fused("", default=False) is False
    assert quant.parse_ldlq_fused("0", default=False) is False and quant.parse_ldlq_fused("1", default=False) is True
    for value, want in ((None, False), ("0", False), ("1", True)):
        monkeypatch.setattr(quant, "_LDLQ_FUSED_RVQ", None)
        if value is None:
            monkeypatch.delenv("QUIP_LDLQ_FUSED_RVQ", raising=False)
        else:
            monkeypatch.setenv("QUIP_LDLQ_FUSED_RVQ", value)
        assert quant.ldlq_fused_rvq_enabled() is want
    monkeypatch.setenv("QUIP_LDLQ_FUSED_RVQ", "0")
    assert quant.ldlq_fused_rvq_enabled() is True                            # read once per process


class _OnGpu:
    """what ldlq_route reads of a tensor, claiming to be an fp32 GPU tensor"""
    is_cuda, dtype = True, torch.float32


@pytest.mark.parametrize("cbid", R.CBIDS)
def test_route(cbid, monkeypatch):
    cb, e8p = R.RvqOracleCodebook(cbid), C.OracleCodebook()
    W = torch.zeros(4, 16)

    def switches(fused, rvq):
        monkeypatch.setattr(quant, "_LDLQ_FUSED", None)
        monkeypatch.setattr(quant, "_LDLQ_FUSED_RVQ", None)
        for name, value in (("QUIP_LDLQ_FUSED", fused), ("QUIP_LDLQ_FUSED_RVQ", rvq)):
            if value is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, value)

    switches(None, None)                                                      # the default: nothing changes
    assert quant.ldlq_route(_OnGpu(), cb) == "stepwise" and quant.ldlq_route(_OnGpu(), e8p) == "panels"
    assert quant.ldlq_route(W, cb) == "stepwise" and quant.ldlq_route(W, e8p) == "stepwise"
    switches(None, "0")
    assert quant.ldlq_route(_OnGpu(), cb) == "stepwise" and quant.ldlq_route(_OnGpu(), e8p) == "panels"
    switches(None, "1")
    assert quant.ldlq_route(_OnGpu(), cb) == "panels" and quant.ldlq_route(_OnGpu(), e8p) == "panels"
    assert quant.ldlq_route(W, cb) == "stepwise" and quant.ldlq_route(W.double(), cb) == "stepwise"      # the CPU
    half = _OnGpu()
    half.dtype = torch.float16
    assert quant.ldlq_route(half, cb) == "stepwise"
    other = R.RvqOracleCodebook(cbid)
    other.id = "D4"
    assert quant.ldlq_route(_OnGpu(), other) == "stepwise"
    switches("0", "1")                                                        # the first switch turns every fused route off
    assert quant.ldlq_route(_OnGpu(), cb) == "stepwise" and quant.ldlq_route(_OnGpu(), e8p) == "stepwise"
    switches("1", None)
    assert quant.ldlq_route(_OnGpu(), cb) == "stepwise" and quant.ldlq_route(_OnGpu(), e8p) == "panels"


def test_panel_launch_refuses_other_codebooks():
    cb = R.RvqOracleCodebook("E8P12RVQ4B")
    cb.id, cb.grid_packed_abs = "D4", None
    with pytest.raises(ValueError):
        quant.panel_launch(cb, torch.device("cpu"))


# ---- the panel arithmetic ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case384():
    W, H = C.make_case(40, 384)
    Wt, Ht = torch.from_numpy(W).double(), torch.from_numpy(H).double()
    return Wt, Ht, torch.linalg.cholesky(Ht)


@pytest.mark.parametrize("iters", [0, 1])
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_panel_recursion_reproduces_stepwise_ldlq(case384, cbid, iters):
    """tests/test_quantize_model_host.py::test_panel_recursion_reproduces_stepwise_ldlq for the two-stage step: the torch
    model of ldlq_panel_rvq driven by quant.LDLQ_panels against quant.LDLQ_stepwise, both in float64 with the brute force
    as the search of each stage.  The indices are equal, or a single row whose tie resolved differently is of equal
    distance to the stepwise target."""
    W, H, L = case384
    cb = R.RvqOracleCodebook(cbid)
    hat_s, q_s = quant.LDLQ_stepwise(W.clone(), H.clone(), L.clone(), cb, iters)
    hat_p, q_p = quant.LDLQ_panels(W.clone(), H.clone(), L.clone(), cb, iters, panel_fn=R.panel_model_rvq(cb))
    assert q_s.dtype == q_p.dtype == torch.int32
    diff = (q_s != q_p).nonzero()
    if len(diff):
        row, col = (int(v) for v in diff[diff[:, 1].argmax()])          # the first group rounded (rightmost) that differs
        assert iters == 0, "ties are settled in the main pass"
        Lb = quant.block_LDL(L.clone(), 8)
        lo, hi = 8 * col, 8 * col + 8
        t = W[row, lo:hi] + (W[row, hi:] - hat_s[row, hi:]) @ Lb[hi:, lo:hi]
        d_s, d_p = (t - hat_s[row, lo:hi]).norm().item(), (t - hat_p[row, lo:hi]).norm().item()
        assert abs(d_s - d_p) <= 1e-12, (row, col, d_s, d_p)
        keep = torch.ones(W.shape[0], dtype=torch.bool)
        keep[diff[:, 0].unique()] = False                                  # rows without a tie must agree entirely
        assert torch.equal(q_s[keep], q_p[keep])
        assert (~keep).sum() <= 1
    else:
        assert torch.equal(hat_s, hat_p)


_STEPWISE = {}


def _stepwise_fp32(cbid, m, n, iters):
    key = (cbid, m, n, iters)
    if key not in _STEPWISE:
        W, H = C.make_case(m, n)
        L64 = C.chol64(H)
        Wt, Ht, Lt = torch.from_numpy(W), torch.from_numpy(H), torch.from_numpy(L64.astype(np.float32))
        hat, Q = quant.LDLQ_stepwise(Wt.clone(), Ht.clone(), Lt.clone(), R.RvqOracleCodebook(cbid), iters)
        _STEPWISE[key] = (W, H, L64, hat.numpy(), Q.numpy())
    return _STEPWISE[key]


@pytest.mark.parametrize("m,n", C.SHAPES)
@pytest.mark.parametrize("cbid", R.CBIDS)
def test_stepwise_fp32_meets_the_float64_step_checks(cbid, m, n):
    """what tests/test_gpu_ldlq_panel_rvq.py asks of the kernel, main pass and tune sweep, met with no exception by the
    repository's own fp32 stepwise loop on the CPU"""
    W, H, L64, hat0, Q0 = _stepwise_fp32(cbid, m, n, 0)
    rep = R.check_rvq_steps(cbid, W, C.O.block_ldl(L64, 8), hat0, Q0)
    print(f"stepwise fp32 {cbid} ({m}, {n}) main pass: {rep}")
    assert rep.steps == m * (n // 8) and rep.over == 0
    assert np.array_equal(hat0, R.decode_f32(cbid, Q0, R.DEFAULT_SCALE[cbid]).reshape(m, n))
    _, _, _, hat1, Q1 = _stepwise_fp32(cbid, m, n, 1)
    rep = R.check_rvq_tune_steps(cbid, W, H, hat0, hat1, Q1)
    print(f"stepwise fp32 {cbid} ({m}, {n}) tune sweep: {rep}")
    assert rep.steps == m * (n // 8) and rep.over == 0


def test_step_check_notices_a_wrong_stage():
    """the check is not vacuous: a second-stage code replaced by another entry, or a hat that is not its codes' decode, counts"""
    cbid = "E8P12RVQ3B"
    W, H, L64, hat, Q = _stepwise_fp32(cbid, 5, 8, 0)
    Lb = C.O.block_ldl(L64, 8)
    assert R.check_rvq_steps(cbid, W, Lb, hat, Q).over == 0
    Q2 = Q.copy()
    Q2[0, 0] = (Q2[0, 0] & ~0xff) | ((Q2[0, 0] & 0xff) ^ 0x80)
    rep = R.check_rvq_steps(cbid, W, Lb, hat, Q2)
    assert rep.hat_wrong == 1
    hat2 = R.decode_f32(cbid, Q2, R.DEFAULT_SCALE[cbid]).reshape(5, 8)
    rep = R.check_rvq_steps(cbid, W, Lb, hat2, Q2)
    assert rep.hat_wrong == 0 and rep.over2 == 1 and rep.over1 == 0
