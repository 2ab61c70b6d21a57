"""Scoring without a GPU: the window plan of the perplexity protocol (exhaustively), the C ABI of the scoring tail
(declared, bound, argument checks before any launch), the shapes of quip_lib::nll_rows's fake, and the build-time invariant of
the kernel: a thread keeps groups of the row in registers between its two passes, and a spill would turn them into scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "quip_nll_rows_f16"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_plan_score_windows_scores_every_target_exactly_once():
    from quip_for_all_amd.score import plan_score_windows
    for n in range(2, 71):
        for window in (2, 3, 8, 16):
            for stride in range(1, window + 1):
                plan = plan_score_windows(n, window, stride)
                scored = [0] * n
                for w, (start, length, first) in enumerate(plan):
                    assert start == w * stride, (n, window, stride)
                    assert 1 <= length <= window and start + length <= n - 1, (n, window, stride)    # rows and their targets exist
                    assert 0 <= first < length, (n, window, stride)                                  # no window without a scored row
                    assert first == (0 if w == 0 else plan[w - 1][0] + plan[w - 1][1] - start)        # where the last window stopped
                    if w and length == window:
                        assert length - first == stride                  # a full later window: its last `stride` rows count
                    for i in range(first, length):
                        scored[start + i + 1] += 1
                assert scored == [0] + [1] * (n - 1), (n, window, stride)
                assert plan[-1][0] + plan[-1][1] == n - 1
                if stride == window:
                    assert all(first == 0 for _, _, first in plan)       # the default: windows that do not overlap
    assert plan_score_windows(10, 4) == plan_score_windows(10, 4, 4) == [(0, 4, 0), (4, 4, 0), (8, 1, 0)]
    assert plan_score_windows(10, 4, 2) == [(0, 4, 0), (2, 4, 2), (4, 4, 2), (6, 3, 2)]


def test_plan_score_windows_refuses_bad_arguments():
    from quip_for_all_amd.score import plan_score_windows
    for kw in (dict(window=1), dict(window=0), dict(window=8, stride=0), dict(window=8, stride=-1), dict(window=8, stride=9),
               dict(window=16, max_len=15), dict(n_tokens=1, window=8), dict(n_tokens=0, window=8)):
        with pytest.raises(ValueError, match="plan_score_windows"):
            plan_score_windows(**{"n_tokens": 20, **kw})
    assert plan_score_windows(20, 16, max_len=16)[0] == (0, 16, 0)


def test_header_and_binding_hold_the_symbol(lib):
    from quip_for_all_amd import capi
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert NAME in set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 13
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME]) == 8 and hasattr(lib, NAME)


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p16 = (ctypes.addressof(buf) + 15) & ~15
    f = lib.quip_nll_rows_f16
    assert f(p16, 0, 8, p16, p16, p16, p16, None) == -2                  # rows < 1
    assert f(p16, -1, 8, p16, p16, p16, p16, None) == -2
    assert f(p16, 2, 0, p16, p16, p16, p16, None) == -2                  # n < 1
    assert f(p16, 2, 0, p16, p16, None, None, None) == -2                # ... also without the optional outputs
    assert f(None, 2, 8, p16, p16, p16, p16, None) == -1                 # logits
    assert f(p16, 2, 8, None, p16, p16, p16, None) == -1                 # target
    assert f(p16, 2, 8, p16, None, p16, p16, None) == -1                 # logprob
    assert f(p16 + 1, 2, 8, p16, p16, p16, p16, None) == -3              # logits: 2-byte aligned
    assert f(p16, 2, 8, p16 + 4, p16, p16, p16, None) == -3              # target: 8
    assert f(p16, 2, 8, p16, p16 + 2, p16, p16, None) == -3              # logprob: 4
    assert f(p16, 2, 8, p16, p16, p16 + 2, p16, None) == -3              # lse: 4
    assert f(p16, 2, 8, p16, p16, p16, p16 + 4, None) == -3              # argmax: 8


def test_nll_rows_fake_and_cpu_refusal():
    import quip_for_all_amd.score  # noqa: F401  (defines the op)
    logits = torch.empty(5, 33, dtype=torch.float16, device="meta")
    out = torch.ops.quip_lib.nll_rows(logits, torch.empty(5, dtype=torch.int64, device="meta"))
    assert [(tuple(o.shape), o.dtype, o.device.type) for o in out] == \
        [((5,), torch.float32, "meta"), ((5,), torch.float32, "meta"), ((5,), torch.int64, "meta")]
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel, no fallback
        torch.ops.quip_lib.nll_rows(torch.zeros(2, 8, dtype=torch.float16), torch.zeros(2, dtype=torch.int64))


def test_decoders_have_the_scoring_methods():
    from quip_for_all_amd.batch_decode import BatchDecoder
    from quip_for_all_amd.decode import LlamaDecoder
    assert callable(LlamaDecoder.score) and callable(LlamaDecoder.perplexity) and callable(BatchDecoder.score_slots)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_nll_rows_kernels_use_no_scratch_and_only_the_reduction_partials_of_lds():
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "nll_rows_kernel" in name):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(scratch) == 2 and len(lds) == 2, "resource remarks of the two instantiations (4 and 8 kept groups) not found"
    assert all(v == 0 for v in scratch.values()), scratch
    assert all(v == 3 * 16 * 4 for v in lds.values()), lds               # 16 wave partials of the maximum, its index and the sum
