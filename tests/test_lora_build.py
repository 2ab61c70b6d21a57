"""Build-time invariants of the LoRA launches (csrc/lora_rows.hip.h, compiled inside decode_glue.hip): the three input
modes of lora_shrink_rows_kernel and lora_expand_rows_kernel exist, each exactly once, and none of them uses scratch (the
expand launch picks its segment out of its argument block without an indexed array).  Only the compiler's resource
remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_lora_kernels_exist_and_use_no_scratch():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, res = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"),
                         ("vgprs", r"VGPRs: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    for mode in (0, 1, 2):
        ks = [n for n in res if "lora_shrink_rows_kernelILi%dEEE" % mode in n]
        assert len(ks) == 1 and res[ks[0]]["scratch"] == 0, (mode, ks, [res[k] for k in ks])
        assert res[ks[0]]["lds"] == 0, res[ks[0]]               # (the staged row is dynamic LDS: sized by the launch)
        assert res[ks[0]]["vgprs"] <= 128, res[ks[0]]           # (512 threads per workgroup)
    ks = [n for n in res if "lora_expand_rows_kernel" in n]
    assert len(ks) == 1 and res[ks[0]]["scratch"] == 0, (ks, [res[k] for k in ks])
