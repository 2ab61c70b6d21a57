"""Build-time invariants of the two paged attention launches on an FP8 cache (csrc/paged_attn.hip.h, compiled inside
decode_glue.hip): both kernels exist for head sizes 64 and 128, converting the cached bytes costs no scratch, and the
static LDS is no more than the fp16 paged kernel's of the same head size (the fp8 chunk becomes the fp16 chunk before it
reaches LDS; the decode kernel's table row is dynamic LDS in both).  Only the compiler's resource remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fp8_paged_attention_kernels_exist_and_use_no_scratch():
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
    # (fp8 kernel, fp16 paged kernel): told apart by the kernel name / the argument struct, not by a template parameter
    pairs = {"ragged": ("rope_attn_paged_ragged_f8_kernelILi%dEEE", "rope_attn_paged_ragged_kernelILi%dEEE"),
             "decode": ("rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb1ENS0_15PagedAttnArgsF8E",
                        "rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb1ENS0_13PagedAttnArgsE")}
    for what, (fp8, fp16) in pairs.items():
        for hd in (64, 128):
            new = [n for n in scratch if fp8 % hd in n]
            old = [n for n in scratch if fp16 % hd in n]
            assert len(new) == 1 and len(old) == 1, (what, hd, sorted(scratch))
            assert scratch[new[0]] == 0, (what, hd, scratch[new[0]])
            assert lds[new[0]] <= lds[old[0]], (what, hd, lds[new[0]], lds[old[0]])
