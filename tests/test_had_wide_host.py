"""Host side of the fp32 / fp64 incoherence transform (no GPU): the C entry's header and refusals, the
QUIP_INCOHERENCE_FUSED switch, the torch branch of incoherence_in / incoherence_out and the kernel's resource remarks."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from quip_for_all_amd import capi, quant

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_header_exports_and_binding_agree():
    src = open(os.path.join(ROOT, "include", "quip_mi355.h")).read()
    abi = int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1))
    decl = " ".join(re.search(r"int quip_had_wide_rows\(([^;]*)\);", src).group(1).split())
    assert decl == ("void* y, const void* x, int32_t dtype, int64_t rows, int32_t in_cols, int32_t out_cols, int32_t n, "
                    "int32_t K, const float* hadK, int32_t hadK_t, const void* s_in, const void* s_out, double scale, "
                    "int32_t store_t, quip_stream_t stream")
    assert abi >= 28 and capi.lib().quip_abi_version() == abi
    assert len(capi.SIGNATURES["quip_had_wide_rows"]) == decl.count(",") + 1


@pytest.mark.parametrize("change,code", [
    ({"y": None}, -1), ({"x": None}, -1), ({"hadK": None}, -1), ({"rows": 0}, -2), ({"K": 0}, -2), ({"n": 200}, -2),
    ({"n": 288, "in_cols": 288, "out_cols": 288}, -2), ({"in_cols": 0}, -2), ({"in_cols": 193}, -2), ({"out_cols": 0}, -2),
    ({"out_cols": 193}, -2), ({"x": 8 + 4096}, -3), ({"y": 4}, -3), ({"x": 1024}, -2), ({"x": 0}, -2),
    ({"dtype": 0}, -5), ({"dtype": 4}, -5), ({"K": 6, "n": 192}, -5), ({"K": 96, "n": 96 * 64}, -5),
    ({"K": 3, "n": 3 * 16384, "in_cols": 8, "out_cols": 8}, -5)])
def test_refusals_come_before_any_device_work(change, code):
    """host memory stands in for the device buffers: a refused call never reads them.  An integer for a pointer: that offset
    into the block; y at 0 holds 2 x 192 fp32 = 1536 bytes, so x at 1024 overlaps it"""
    buf = (ctypes.c_char * 16384)()
    base = (ctypes.addressof(buf) + 15) & ~15
    a = dict(y=0, x=4096, hadK=8192, dtype=2, rows=2, in_cols=192, out_cols=192, n=192, K=3)
    a.update(change)
    y, x, hadK = (None if a[k] is None else base + a[k] for k in ("y", "x", "hadK"))
    assert capi.lib().quip_had_wide_rows(y, x, a["dtype"], a["rows"], a["in_cols"], a["out_cols"], a["n"], a["K"], hadK, 0,
                                         None, None, 1.0, 0, None) == code


@pytest.mark.parametrize("value,on", [(None, False), ("", False), ("0", False), ("1", True)])
def test_switch_is_off_unless_set(value, on, monkeypatch):
    monkeypatch.setattr(quant, "_INCOHERENCE_FUSED", None)
    (monkeypatch.delenv("QUIP_INCOHERENCE_FUSED", raising=False) if value is None
     else monkeypatch.setenv("QUIP_INCOHERENCE_FUSED", value))
    assert quant.incoherence_fused_enabled() is on
    monkeypatch.setenv("QUIP_INCOHERENCE_FUSED", "0" if on else "1")
    assert quant.incoherence_fused_enabled() is on, "read once per process"


def test_cpu_tensors_take_the_expressions_they_replaced(monkeypatch):
    monkeypatch.setattr(quant, "_INCOHERENCE_FUSED", True)       # CPU tensors take the torch branch whatever the switch says
    g = torch.Generator().manual_seed(5)
    rows, columns, lK, lN, rK, rN = 50, 150, 3, 192, 1, 64      # K > 1 and in_cols < n on the left, padding on the right
    lhad, rhad = torch.linalg.qr(torch.randn(3, 3, generator=g))[0].contiguous(), None
    H, w, hat = (torch.randn(s, generator=g) for s in ((columns, columns), (rows, columns), (rN, lN)))
    SU, SV = torch.randn(columns, generator=g).sign(), torch.randn(rows, generator=g).sign()
    hU, hUt = quant.matmul_hadU, quant.matmul_hadUt
    Hi, wi = quant.incoherence_in(H, w, SU, SV, lhad, lK, lN, rhad, rK, rN)
    assert torch.equal(Hi, hUt(hUt(H * SU, lhad, lK, lN).T * SU, lhad, lK, lN))
    assert torch.equal(wi, hUt(hUt(w.T * SV, rhad, rK, rN).T * SU, lhad, lK, lN))
    out = quant.incoherence_out(hat, SU, SV, lhad, lK, lN, rhad, rK, rN, columns, rows)
    assert torch.equal(out, (hU((hU(hat, lhad, lK, lN)[..., :columns] * SU).T, rhad, rK, rN)[..., :rows] * SV).T)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_no_instantiation_uses_scratch():
    src = os.path.join(ROOT, "quip_for_all_amd", "csrc", "had_wide.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "had_wide_rows_kernel" in name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 11 and set(scratch.values()) == {0}, scratch      # fp32: CH 1 .. 16, fp64: CH 1 .. 32
