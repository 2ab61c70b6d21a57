"""Build-time invariants of the q / k norm kernels (csrc/qk_norm.hip.h, compiled inside decode_glue.hip): the four
instantiations of rope_attn_decode_kernel that fuse the norm (bs = 1 and contiguous batched, head sizes 64 and 128) and
qk_norm_rows_kernel exist, none of them uses scratch, the fused ones need no more static LDS than their plain
counterparts -- and the plain counterparts are still found exactly once under their names: the norm came as an argument
type, not as one more template parameter.  Only the compiler's resource remarks are read."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_qk_norm_kernels_exist_and_use_no_scratch():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, res = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    for hd in (64, 128):
        rows = [n for n in res if "qk_norm_rows_kernelILi%dEEE" % hd in n]
        assert len(rows) == 1 and res[rows[0]]["scratch"] == 0, (hd, rows)
        for seq in (0, 1):
            fused = [n for n in res if "rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb%dENS0_10QkNormArgsINS0_8AttnArgsEEE"
                     % (hd, seq) in n]
            plain = [n for n in res if "rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb%dENS0_8AttnArgsE" % (hd, seq) in n]
            assert len(fused) == 1 and len(plain) == 1, (hd, seq, sorted(res))
            assert res[fused[0]]["scratch"] == 0, (hd, seq, res[fused[0]])
            assert res[fused[0]]["lds"] <= res[plain[0]]["lds"], (hd, seq, res[fused[0]], res[plain[0]])
