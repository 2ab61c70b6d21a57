"""The device sampler without a GPU: the C ABI of quip_sample_step_f16 (declared, bound, argument checks before any launch),
quip_lib::sample_step's fake, the kernel's build-time resources, and the float64
restatement of the function (sampler.sample_step_ref) against theory: on a small row with ties the frequencies of 8192
draws sit where the probabilities of the kept set say, over positions and over seeds (row and seed bases chosen so that
the oracle's worst |count - N q| is 0.66 of the bound 5 sqrt(N q (1 - q)) + 3; the test prints every case's figure)."""
import ctypes
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "quip_sample_step_f16"
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
KERNEL_SRC = os.path.join(REPO, "quip_for_all_amd", "csrc", "sample_rows.hip.h")


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_header_and_binding_hold_the_symbol(lib):
    from quip_for_all_amd import capi
    src = open(os.path.join(REPO, "include", "quip_mi355.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert NAME in set(re.findall(r"\b(quip_[a-z0-9_]+)\s*\(", src))
    assert int(re.search(r"#define QUIP_ABI_VERSION (\d+)", src).group(1)) >= 17
    assert NAME in capi.SIGNATURES and len(capi.SIGNATURES[NAME]) == 11 and hasattr(lib, NAME)
    assert "sample_rows_launch" in open(os.path.join(REPO, "quip_for_all_amd", "csrc", "quip_internal.h")).read()


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    f = lib.quip_sample_step_f16
    ok = [p, 2, 8, p, p, p, p, p, p, p, None]            # logits rows n temperature top_k top_p seed tok pos kept stream
    for i in (0, 3, 4, 5, 6, 7, 8):                      # every pointer but kept must be there
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == -1, i
    for rows, n in ((0, 8), (-1, 8), (2, 0), (2, -5), (2, (1 << 20) + 1)):
        assert f(p, rows, n, p, p, p, p, p, p, p, None) == -2, (rows, n)
        assert f(p, rows, n, p, p, p, p, p, p, None, None) == -2, (rows, n)       # ... also without kept
    for i, off in ((0, 1), (3, 2), (4, 2), (5, 2), (6, 4), (7, 4), (8, 4), (9, 2)):
        assert f(*[a + off if j == i else a for j, a in enumerate(ok)]) == -3, i  # 2 | 4 4 4 | 8 8 8 | 4 byte alignment


def test_fake_on_meta_and_cpu_refusal():
    import quip_for_all_amd.sampler  # noqa: F401  (defines the op)
    def m(*shape, dtype):
        return torch.empty(*shape, dtype=dtype, device="meta")
    args = (m(5, 33, dtype=torch.float16), m(5, dtype=torch.float32), m(5, dtype=torch.int32), m(5, dtype=torch.float32),
            m(5, dtype=torch.int64), m(5, dtype=torch.int64), m(5, dtype=torch.int64))
    assert torch.ops.quip_lib.sample_step(*args) is None
    assert torch.ops.quip_lib.sample_step(*args, m(5, dtype=torch.int32)) is None
    assert torch.ops.quip_lib.sample_step(*args, kept=None) is None
    z = torch.zeros
    with pytest.raises((NotImplementedError, RuntimeError)):             # no CPU kernel, no fallback
        torch.ops.quip_lib.sample_step(z(2, 8, dtype=torch.float16), z(2), z(2, dtype=torch.int32), z(2),
                                       z(2, dtype=torch.int64), z(2, dtype=torch.int64), z(2, dtype=torch.int64))
    from quip_for_all_amd import register_lib
    assert "sample_step" not in register_lib._SCHEMAS


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_kernel_uses_no_scratch_and_the_lds_its_header_states():
    stated = int(re.search(r"LDS = kSmpLdsBytes = (\d+) bytes", open(KERNEL_SRC).read()).group(1))
    src = os.path.join(REPO, "quip_for_all_amd", "csrc", "decode_glue.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", os.devnull, src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True)
    name, scratch, lds = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        if not (name and "sample_rows_kernel" in name):
            continue
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m:
            scratch[name] = int(m.group(1))
        m = re.search(r"LDS Size \[bytes/block\]: (\d+)", line)
        if m:
            lds[name] = int(m.group(1))
    assert len(scratch) == 1 and len(lds) == 1, "resource remarks of sample_rows_kernel not found"
    assert list(scratch.values()) == [0], scratch
    assert list(lds.values()) == [stated] and stated == 26464, (lds, stated)


def test_delta_of_the_header_is_the_one_the_tests_use():
    from quip_for_all_amd import sampler as S
    log2 = int(re.search(r"kSmpDeltaLog2 = (-\d+)", open(KERNEL_SRC).read()).group(1))
    assert S.DELTA == 2.0 ** log2 and S.DELTA <= 2.0 ** -16
    assert S.MAX_N == 1 << 20


# (seed, pos) -> h, from the definition (also evaluated once in uint64 arithmetic independent of sampler.py)
PINNED_HASHES = [
    (0, 0, 0xA706DD2F4D197E6F),
    (0, 1, 0xB382A305F4414F5E),
    (1, 0, 0x5E41AB087439611E),
    (1, 1, 0xF18D6CE93D6CF1EE),
    (2 ** 62 + 12345, 4095, 0x83396630569D02B7),
    (-1, 0, 0x5DC20AA7B2A27137),
    (0x123456789ABCDEF, 2 ** 40, 0xD14D623EE288287F),
    (42, 131071, 0xA42A4A7A2B6E19E3),
]


def test_hash_is_pinned():
    from quip_for_all_amd import sampler as S
    G = 0x9E3779B97F4A7C15
    assert S._mix(G) == 0xE220A8397B1DCDAF               # splitmix64 seeded with 0: its first output
    for seed, pos, h in PINNED_HASHES:
        assert S.sample_hash(seed, pos) == h, (seed, pos, hex(S.sample_hash(seed, pos)))
        assert S.sample_uniform(seed, pos) == ((h >> 40) + 0.5) * 2.0 ** -24
    # the seed is mixed before the counter: consecutive seeds at one position and consecutive positions of one seed
    # both give uniforms without a visible step
    for us in ([S.sample_uniform(s, 7) for s in range(4096)], [S.sample_uniform(7, c) for c in range(4096)]):
        us = np.array(us)
        assert 0.0 < us.min() and us.max() < 1.0
        assert abs(us.mean() - 0.5) < 5 * math.sqrt(1 / 12 / 4096)
        assert abs(np.corrcoef(us[:-1], us[1:])[0, 1]) < 5 / math.sqrt(4096)


ROW = [2.0, 1.0, 2.0, 0.5, -60000.0, 1.0, 0.0, -1.0, 1.0, 3.0, -2.5]     # ties at 2 and at 1, one entry without mass
SETTINGS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.0, 0, 0.8), (1.5, 8, 0.9)]   # (T, k, p)
N_DRAWS = 8192


def _theory(row, T, k, p):
    """the probabilities of the kept set, by the rules of DESIGN 4.16 spelled out with loops -> {token: q}"""
    vals = sorted(set(row), reverse=True)
    if 1 <= k < len(row):
        kth = sorted(row, reverse=True)[k - 1]
        vals = [v for v in vals if v >= kth]
    mass = {v: row.count(v) * math.exp((v - vals[0]) / T) for v in vals}
    if 0.0 < p < 1.0:
        zk, above, kept = sum(mass.values()), 0.0, []
        for v in vals:
            if not kept or above < p * zk:
                kept.append(v)
            above += mass[v]
        vals = kept
    z = sum(mass[v] for v in vals)
    return {i: math.exp((x - vals[0]) / T) / z for i, x in enumerate(row) if x in vals}


def _worst_ratio(counts, q):
    """max over tokens of |count - N q| / (5 sqrt(N q (1 - q)) + 3)"""
    return max(abs(counts.get(t, 0) - N_DRAWS * qt) / (5 * math.sqrt(N_DRAWS * qt * (1 - qt)) + 3) for t, qt in q.items())


@pytest.mark.parametrize("T,k,p", SETTINGS)
def test_reference_draws_follow_the_kept_distribution(T, k, p):
    from quip_for_all_amd import sampler as S
    q = _theory(ROW, T, k, p)
    assert abs(sum(q.values()) - 1.0) < 1e-12
    dist = S.sample_dist_ref(np.array(ROW, dtype=np.float16), T, k, p)
    assert dist["kept"] == len(q) and sorted(dist["order"].tolist()) == sorted(q)
    assert q.get(4, 0.0) == 0.0                                           # the -60000 entry: finite, so kept unless cut; no mass
    for what, draws in (("positions", [(1234, c) for c in range(N_DRAWS)]), ("seeds", [(s, 77) for s in range(N_DRAWS)])):
        counts = {}
        for seed, pos in draws:
            t = S.sample_draw_ref(dist, seed, pos)
            counts[t] = counts.get(t, 0) + 1
        assert set(counts) <= set(q), (what, set(counts) - set(q))       # nothing outside the kept set
        assert 4 not in counts
        ratio = _worst_ratio(counts, q)
        print(f"T={T} k={k} p={p} over {what}: worst |count - N q| / bound = {ratio:.3f}")
        assert ratio <= 1.0, (what, ratio)


def test_reference_rules_on_small_rows():
    from quip_for_all_amd import sampler as S
    x = np.array([1.0, 3.0, 3.0, -np.inf, np.nan, 2.0, 2.0, 0.0], dtype=np.float16)
    d = S.sample_dist_ref(x, 1.0, 0, 1.0)
    assert d["order"].tolist() == [1, 2, 5, 6, 0, 7] and d["kept"] == 6           # canonical order; NaN / -inf never
    assert S.sample_dist_ref(x, 1.0, 3, 1.0)["order"].tolist() == [1, 2, 5, 6]    # ties at the k-th value all stay
    assert S.sample_dist_ref(x, 1.0, 2, 1.0)["order"].tolist() == [1, 2]
    assert S.sample_dist_ref(x, 1.0, 0, 0.5)["order"].tolist() == [1, 2]          # class 1 holds 0.62 of the mass
    assert S.sample_dist_ref(x, 1.0, 0, 0.7)["order"].tolist() == [1, 2, 5, 6]    # ties are never split
    for T in (0.0, -1.0, float("nan")):
        assert S.sample_dist_ref(x, T, 0, 1.0) == {"greedy": True, "token": 1, "kept": 1, "margin": math.inf}
    assert S.sample_dist_ref(np.array([1, np.inf, 2], dtype=np.float16), 1.0, 0, 1.0)["token"] == 1
    assert S.sample_dist_ref(np.array([np.nan, np.nan], dtype=np.float16), 1.0, 0, 1.0)["token"] == 0
    assert S.sample_dist_ref(np.array([-np.inf, -np.inf], dtype=np.float16), 1.0, 0, 1.0)["token"] == 0
    d = S.sample_dist_ref(np.array([0.0, -0.0, -1.0], dtype=np.float16), 1.0, 0, 1.0)
    assert d["order"].tolist() == [0, 1, 2] and abs(d["cum"][1] - 2.0) < 1e-15    # -0 is +0
    r = S.sample_step_ref(torch.tensor([ROW, ROW], dtype=torch.float16), [1.0, 0.0], [0, 0], [0.8, 1.0], [5, 5], [9, 9])
    assert r[1]["greedy"] and r[1]["token"] == 9
    i = r[0]["order"].tolist().index(r[0]["token"])
    assert r[0]["lo"][i] <= r[0]["u"] * r[0]["Z"] < r[0]["hi"][i] and S.sample_accepts(r[0], r[0]["token"], 5, 9)
    assert not S.sample_accepts(r[0], 4, 5, 9)
