"""Build-time invariant of the chunk attention launch (csrc/chunk_attn.hip.h, compiled inside decode_glue.hip): both
head-dim instantiations hold the output tile, the query fragments and a tile's scores in registers -- a spill would
turn the tile loop into scratch traffic.  LDS stays far below the 160 KiB of a CU."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_chunk_attention_kernels_use_no_scratch():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "rope_attn_chunk_kernel" in name):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(scratch) == 2 and len(lds) == 2, "resource remarks of the two instantiations (head_dim 64, 128) not found"
    assert any("ILi64E" in n for n in scratch) and any("ILi128E" in n for n in scratch)
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(v <= 160 * 1024 for v in lds.values()), lds
