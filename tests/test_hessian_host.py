"""Host side of the fused Hessian accumulation (no GPU): the C entry's header and refusals, the QUIP_HESSIAN_FUSED switch and
the rule by which quantize_model's hooks accumulate a shared input once."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

from quip_for_all_amd import capi, quip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_exports_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "quip_mi355.h")).read()
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    decl = " ".join(re.search(r"int quip_hessian_accumulate_f64\(([^;]*)\);", src).group(1).split())
    assert decl == ("void* H, void* mu, const void* x, int32_t x_dtype, int64_t rows, int32_t n, double keep, double s_h, "
                    "double s_mu, quip_stream_t stream")
    assert abi >= 27 and capi.lib().quip_abi_version() == abi
    assert len(capi.SIGNATURES["quip_hessian_accumulate_f64"]) == decl.count(",") + 1
    assert capi.lib().quip_hessian_row_block() == int(re.search(r"#define QUIP_HESSIAN_ROW_BLOCK (\d+)", src).group(1))


@pytest.mark.parametrize("change,code", [
    ({"H": None}, -1), ({"mu": None}, -1), ({"x": None}, -1), ({"n": 12}, -2), ({"n": 0}, -2), ({"rows": 0}, -2),
    ({"rows": -3}, -2), ({"dtype": 3}, -5), ({"dtype": -1}, -5), ({"x": 8}, -3), ({"H": 4}, -3), ({"mu": 4}, -3)])
def test_refusals_come_before_any_device_work(change, code):
    """host memory stands in for the device buffers: a refused call never reads them.  An integer for a pointer: that offset"""
    buf = (ctypes.c_char * 256)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a = dict(H=0, mu=0, x=0, dtype=2, rows=4, n=16)
    a.update(change)
    H, mu, x = (None if a[k] is None else base + a[k] for k in ("H", "mu", "x"))
    assert capi.lib().quip_hessian_accumulate_f64(H, mu, x, a["dtype"], a["rows"], a["n"], 0.5, 0.5, 0.25, None) == code


@pytest.mark.parametrize("value,on", [(None, False), ("", False), (" ", False), ("0", False), ("1", True), ("yes", True)])
def test_switch_is_off_unless_set(value, on, monkeypatch):
    monkeypatch.setattr(quip, "_HESSIAN_FUSED", None)
    monkeypatch.delenv("QUIP_HESSIAN_FUSED", raising=False) if value is None else monkeypatch.setenv("QUIP_HESSIAN_FUSED", value)
    assert quip.hessian_fused_enabled() is on
    monkeypatch.setenv("QUIP_HESSIAN_FUSED", "0" if on else "1")
    assert quip.hessian_fused_enabled() is on, "read once per process"


@pytest.mark.parametrize("second,copies", [("same", 1), ("equal", 0), ("modified", 0), ("view", 0)])
def test_shared_inputs_accumulate_once(second, copies):
    x = torch.randn(2, 5, 16)
    first, other, alone = (quip.QUIP(nn.Linear(16, 4), nn.Identity()) for _ in range(3))
    shared = quip.SharedHessianInputs()
    for batch in range(2):                                # the second batch: both modules carry a history by then
        shared.add_batch(first, x)
        if second == "modified":
            x.add_(1.0)
        y = {"equal": x.clone(), "view": x[:, :4]}.get(second, x)
        shared.add_batch(other, y)
        alone.add_batch(y)
        assert shared.copies == copies * (batch + 1)
        assert torch.equal(other.H, alone.H) and torch.equal(other.mu, alone.mu) and other.nsamples == alone.nsamples
        assert other.H.data_ptr() != first.H.data_ptr()
        x = torch.randn(2, 5, 16)
    narrow = quip.QUIP(nn.Linear(8, 4), nn.Identity())   # other columns never share, whatever the tensor
    shared.add_batch(first, x)
    with pytest.raises(RuntimeError):
        shared.add_batch(narrow, x)
    assert shared.copies == 2 * copies
