"""decode_block_tiled.hip: the Llama-2-7B-shaped persistent launch compiled for the launch-tiled layout of the codes (codebook id 5).
Build-time invariants of the new translation unit and the argument checks of its host entry points; no GPU needed."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
# the shipped E8P12 nibble instantiation of decode_block.hip (the kernel this one replaces at run time): profiles/tiled7b_resources.txt
PARENT_NIBBLE_VGPRS = 240


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_tiled_block_engine_kernel_uses_no_scratch_and_touches_no_register_in_flight():
    """one instantiation (E8P12 in nibble mode); no scratch (a spill is a VMEM operation the hand-counted waits do not know), no
    instruction on an in-flight register, no more VGPRs than the row-major kernel and two waves per SIMD; every weight request of the
    kernel is one of the tiled pattern's: no load with the row-major second-half offset is left"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_inflight
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_block_tiled.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", "-", src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True, cwd=os.path.dirname(src))
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert scratch == [0], scratch
    assert [int(x) for x in re.findall(r" VGPRs: (\d+)", r.stderr)][0] <= PARENT_NIBBLE_VGPRS
    assert [int(x) for x in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", r.stderr)] == [2]
    kernels = [(n, l) for n, l in check_inflight.kernels_of(r.stdout) if "decode_block_kernel" in n]
    assert len(kernels) == 1
    name, lines = kernels[0]
    assert check_inflight.check_kernel(lines) == [], name
    # the weight requests: scalar base + 32-bit lane offset, `nt`
    loads = [l for l in lines if re.search(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\].* nt", l)]
    assert len(loads) >= 26                                   # 13 items of two requests each
    offs = [int(m.group(1), 0) if m else 0 for m in (re.search(r"offset:(\S+)", l) for l in loads)]
    assert 64 not in offs, "a row-major request in the tiled kernel"
    assert set(offs) == {0, 1024, 704}, sorted(set(offs))     # (704 = 11 rows x 64 bytes: gate / up's short row block)
    assert offs.count(704) == 2

def test_entry_points_check_their_arguments_without_a_gpu():
    """every rejection comes before a launch"""
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    L = capi.lib()
    buf = (ctypes.c_char * (4 * 256 * 64 + 64))()
    p = (ctypes.addressof(buf) + 15) & ~15
    n = 256 * 64
    for fn in (L.quip_tile_codes_view, L.quip_untile_codes_view):
        assert fn(None, p, 256, 64, None) == -1 and fn(p, None, 256, 64, None) == -1
        assert fn(p, p + n, 255, 64, None) == -2           # rows % 256
        assert fn(p, p + n, 11008 + 16, 64, None) == -2
        assert fn(p, p + n, 256, 96, None) == -2           # row_bytes % 64
        assert fn(p, p + n, -256, 64, None) == -2
        assert fn(p + 8, p + 2 * n, 256, 64, None) == -3   # misaligned source
        assert fn(p, p + n + 8, 256, 64, None) == -3       # misaligned destination
        assert fn(p, p, 256, 64, None) == -5               # in place
        assert fn(p, p + n // 2, 256, 64, None) == -5      # partial overlap
        assert fn(p + n // 2, p, 256, 64, None) == -5
        assert fn(p, p + n, 0, 64, None) == 0              # empty: ok, no launch
    # codebook id 5 is shape 0's: the other two launches refuse it
    p64 = (ctypes.addressof(buf) + 63) & ~63
    for shape in (1, 2):
        a = capi.BlockEngineArgs(p64, p64, p64, p64, p64, p64, p64, p64, None, 1, 16, -1, 1e-5, 0.1, 5, 0.0, shape, None)
        assert L.quip_block_engine(ctypes.byref(a), None) == -5
        t = capi.TokenTailArgs(p64, p64, p64, p64, p64, p64, None, 2048)
        assert L.quip_block_engine_token(ctypes.byref(a), ctypes.byref(t), None) == -5
