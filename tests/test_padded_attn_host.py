"""The padded batched decode launch without a GPU: the C ABI entry (declared, bound, every refusal before any launch), the
op's schema and fake, what a padded BatchDecoder refuses, and the build-time invariant that the two new instantiations of
the decode kernel use no scratch and no more waves-per-SIMD-limiting registers than their siblings (compiler remarks)."""
import ctypes
import os
import re
import shutil
import subprocess
import types

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "quip_rope_attn_decode_batched_start_f16"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_declares_the_entry_and_the_abi_version_moved():
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert ENTRY in set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 18


def test_python_binding_covers_the_entry(lib):
    from quip_for_all_amd import capi
    batched = capi.SIGNATURES["quip_rope_attn_decode_batched_f16"]
    assert capi.SIGNATURES[ENTRY] == batched + [ctypes.c_void_p]          # the batched entry's list plus `start`
    assert hasattr(lib, ENTRY)
    assert lib.quip_abi_version() >= 18


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15

    def call(*, q=p16, out=p16, pos=p16, start=p16, kcache=p16, ws=None, batch=4, heads=4, kvh=2, hd=64, max_len=128,
             window=0):
        return lib.quip_rope_attn_decode_batched_start_f16(q, p16, p16, p16, p16, pos, kcache, p16, out, batch, heads, kvh,
                                                           hd, max_len, 0.125, window, ws, None, start)
    assert call(q=None) == -1 and call(out=None) == -1 and call(pos=None) == -1 and call(kcache=None) == -1
    assert call(start=None) == -1
    assert call(batch=0) == -2 and call(batch=65536) == -2 and call(heads=6, kvh=4) == -2 and call(max_len=0) == -2
    assert call(window=-1) == -2
    assert call(hd=96) == -5
    assert call(q=p16 + 2) == -3 and call(kcache=p16 + 8) == -3 and call(pos=p16 + 4) == -3 and call(start=p16 + 4) == -3
    assert call(ws=p16 + 8) == -3


def test_op_schema_and_fake_on_meta_tensors():
    import quip_for_all_amd.batch_decode  # noqa: F401  (defines the op)
    op = torch.ops.quip_lib.rope_attn_decode_batched_start
    names = [a.name for a in op.default._schema.arguments]
    assert names == ["q", "k", "v", "cos", "sin", "pos", "start", "kcache", "vcache", "workspace", "window"]
    old = [a.name for a in torch.ops.quip_lib.rope_attn_decode_batched.default._schema.arguments]
    assert old == [n for n in names if n != "start"]                     # the existing op's schema did not change
    m = lambda *s, dtype=torch.float16: torch.empty(*s, dtype=dtype, device="meta")  # noqa: E731
    kc = m(3, 2, 32, 64)
    out = op(m(3, 8, 64), m(3, 2, 64), m(3, 2, 64), m(32, 64, dtype=torch.float32), m(32, 64, dtype=torch.float32),
             m(3, dtype=torch.int64), m(3, dtype=torch.int64), kc, kc, None, 0)
    assert out.device.type == "meta" and tuple(out.shape) == (3, 8, 64) and out.dtype == torch.float16


def test_paged_and_padded_together_are_refused():
    from quip_for_all_amd.decode import LlamaDecoder
    with pytest.raises(ValueError, match="padded"):
        LlamaDecoder.batched(types.SimpleNamespace(), 2, paged=True, padded=True)


def test_prompt_side_methods_of_a_padded_decoder_raise():
    """(no device: the refusal comes before anything is touched)"""
    from quip_for_all_amd.batch_decode import BatchDecoder
    bd = object.__new__(BatchDecoder)
    bd.start = torch.zeros(2, dtype=torch.long)
    for call in (lambda: bd.fill_slot(0, [1, 2]), lambda: bd.extend_slot(0, [1]), lambda: bd.prefill_slot(0, [1, 2]),
                 lambda: bd.fill_slots([0], [[1, 2]]), lambda: bd.extend_slots([0], [[1]]),
                 lambda: bd.score_slots([0], [[1, 2]]), lambda: bd.generate([[1], [2]], 2)):
        with pytest.raises(NotImplementedError, match="padded=True"):
            call()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_new_instantiations_use_no_scratch_and_keep_the_siblings_occupancy():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, res = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("lds", r"LDS Size \[bytes/block\]: (\d+)")):
            m = re.search(pat, line)
            if m and name:
                res.setdefault(name, {})[key] = int(m.group(1))
    for hd in (64, 128):
        new = [n for n in res if "rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb1ENS0_13StartAttnArgsE" % hd in n]
        old = [n for n in res if "rope_attn_decode_kernelILi%dELb0ELi0ELi0ELb1ENS0_8AttnArgsE" % hd in n]
        assert len(new) == 1 and len(old) == 1, (hd, sorted(res))
        assert res[new[0]]["scratch"] == 0, (hd, res[new[0]])
        assert res[new[0]]["occ"] >= res[old[0]]["occ"], (hd, res[new[0]], res[old[0]])
        assert res[new[0]]["lds"] <= res[old[0]]["lds"], (hd, res[new[0]], res[old[0]])
