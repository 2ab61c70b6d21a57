"""The grouped skinny kernel's device code (csrc/e8p_skinny_group.hip), compiled for gfx950 without a GPU."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_skinny_group_kernel_touches_no_register_in_flight():
    """e8p_skinny_group_kernel runs the tile body of e8p_skinny_gemm.hip inside a tile loop: the hand-counted vmcnt queue
    must hold across the loop's edge too.  tools/check_inflight.py follows every path of all 20 instantiations (2 x 2 shapes
    x five codebook modes) and may find no instruction that touches the destination of a load still in the queue; no
    instantiation may use scratch (a spill is a vector-memory operation the counts do not know)."""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_inflight
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "e8p_skinny_group.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", "-", src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    assert len(scratch) == 20 and not any(scratch), scratch
    kernels = [(n, l) for n, l in check_inflight.kernels_of(r.stdout) if "e8p_skinny_group_kernel" in n]
    assert len(kernels) == 20
    for name, lines in kernels:
        assert any("global_load_lds_dwordx4" in l for l in lines), name
        assert check_inflight.check_kernel(lines) == [], name
