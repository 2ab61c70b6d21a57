"""The counted waits of the gate / up products (csrc/decode_block.hip: esync::wait_all_but in front of each live item, down's requests
between the multiplies) keep weight requests in flight across more code than the one wait for the whole queue did.  Of
EVERY decode_block_kernel instantiation of the three translation units that compile that file: no scratch (a spill is a vector-memory
operation the hand-counted queue does not know), two waves per SIMD, at most 240 VGPRs on the launch-tiled kernel (the bound
tests/test_tiled7b_build.py states), and no instruction on a register whose load is still in flight (tools/check_inflight.py, which
retires the queue at counted waits).  No GPU needed."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
UNITS = ("decode_block.hip", "decode_block_g8.hip", "decode_block_tiled.hip")
TILED_VGPRS = 240


def _compile(unit):
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", unit)
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", "-", src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True, cwd=os.path.dirname(src))
    return r.stdout, r.stderr


def _resources(remarks):
    """{function: {field: value}} of -Rpass-analysis=kernel-resource-usage"""
    out, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: .*?Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\d+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_every_block_kernel_has_no_scratch_two_waves_and_touches_no_register_in_flight():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_inflight
    with ThreadPoolExecutor(max_workers=len(UNITS)) as ex:
        built = dict(zip(UNITS, ex.map(_compile, UNITS)))
    for unit, (asm, remarks) in built.items():
        res = {n: f for n, f in _resources(remarks).items() if "decode_block_kernel" in n}
        kernels = [(n, l) for n, l in check_inflight.kernels_of(asm) if "decode_block_kernel" in n]
        assert kernels and sorted(res) == sorted(n for n, _ in kernels), (unit, sorted(res))
        assert unit != "decode_block_tiled.hip" or len(kernels) == 1
        for name, lines in kernels:
            f = res[name]
            assert f["ScratchSize [bytes/lane]"] == 0, (unit, name, f)
            assert f["Occupancy [waves/SIMD]"] == 2, (unit, name, f)
            assert f["VGPRs"] <= (TILED_VGPRS if unit == "decode_block_tiled.hip" else 256), (unit, name, f)
            assert check_inflight.check_kernel(lines) == [], (unit, name)
            # the counted waits are there: a kernel with none of them would pass the checks above by waiting for everything
            # (shape 0, <REP, RVQ = false>: the RVQ codebooks, HI and the G8 launch keep their one wait for the whole queue)
            if unit != "decode_block_g8.hip" and re.search(r"decode_block_kernelILi\d+ELb0E", name):
                counted = [int(m.group(1)) for m in (re.search(r"s_waitcnt vmcnt\((\d+)\)", l) for l in lines) if m]
                assert all(c in counted for c in (10, 8, 6)), (unit, name, sorted(set(counted)))
