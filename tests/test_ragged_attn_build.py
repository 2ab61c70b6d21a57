"""Build-time invariant of the ragged attention launch (csrc/ragged_attn.hip.h, compiled inside decode_glue.hip): the
segment scan in front of the chunk launch's tile code reads the segment table from the kernel arguments with scalar
loads -- a copy of the table into private memory would show as scratch -- and the tile code keeps its registers.  LDS is
the chunk kernel's, far below the 160 KiB of a CU.  Only the compiler's resource remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_attention_kernels_use_no_scratch():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not name:
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    ragged = sorted(n for n in scratch if "rope_attn_ragged_kernel" in n)
    assert len(ragged) == 2 and all(n in lds for n in ragged), "resource remarks of the two instantiations (head_dim 64, 128)"
    assert any("ILi64E" in n for n in ragged) and any("ILi128E" in n for n in ragged)
    assert all(scratch[n] == 0 for n in ragged), scratch
    assert all(lds[n] <= 160 * 1024 for n in ragged), lds
    # no more LDS than the chunk kernel of the same head_dim (the tile code is shared, the scan needs none)
    for hd in ("ILi64E", "ILi128E"):
        chunk = [lds[n] for n in lds if "rope_attn_chunk_kernel" in n and hd in n]
        assert len(chunk) == 1 and lds[next(n for n in ragged if hd in n)] <= chunk[0]
