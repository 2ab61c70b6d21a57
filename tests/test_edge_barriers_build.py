"""The 4096-wide edges of the persistent block launch on two exchange buffers (csrc/decode_block.hip: BLds::kBuf1, edge()):
build-time invariants of the translation units that compile that file, and of decode_block_gqa.hip, which shares hadw::fwd / rev.
Of EVERY decode_block_kernel instantiation: no scratch, two waves per SIMD, at most 240 VGPRs on the launch-tiled kernel, and an LDS
map of at most 160 KB -- BLds::kBytes itself, read out of a probe that includes decode_block.hip and stores the map's constants in a
device array.  The kernels whose edges changed hold as many s_barrier instructions fewer than the parent commit's as the design
removes; those that keep one buffer (the virtual rows of RVQ / HI, G8) and the grouped-query kernel hold exactly as many.  No GPU
needed."""
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "quip_for_all_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TILED_VGPRS = 240
LDS_BUDGET = 160 * 1024
# s_barrier instructions in the listings of the PARENT commit (hipcc -O3 -S, gfx950; profiles/edge_barriers_resources.txt)
PARENT_BARRIERS = {"two_buffers": 54, "rvq": 56, "g8": 54, "gqa": 48}
# What the design removes from a kernel with two buffers.  The listing holds three copies of edge():
#   block 0's (no fwd; `two` is a run-time value, so both branches are there):
#       rev<2> leading 1 + rev<1> leading and behind-the-reads 2 + behind the planes 1                          = 4
#   gate / up's (`two` is the literal false: one branch):
#       fwd leading 1 + rev<1> leading and behind-the-reads 2 + behind the planes 1                             = 4
#   q / k / v's (both branches):
#       fwd leading 1 + rev<2> leading 1 + rev<1> leading and behind-the-reads 2 + behind the planes 1          = 5
# Executed per edge: six barriers -> two (one consumer) or three (two consumers: rev<2> keeps the one behind its reads).
REMOVED = 4 + 4 + 5
# the map's constants per instantiation <REP, RVQ>, in the probe's order
PROBE_INSTANCES = [(4, 0), (24, 0), (16, 0), (64, 0), (16, 1), (64, 1), (12, 1)]
PROBE_FIELDS = ("kBytes", "kArea", "kAreaBytes", "kBuf0", "kBuf1", "kBufBytes", "kHad", "kStash", "PSH")


def _compile(src, cwd=CSRC):
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", "-o", "-", src,
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, check=True, cwd=cwd)
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


def _barriers(lines):
    return sum(1 for l in lines if re.search(r"^\s*s_barrier\b", l))


def _probe_source():
    """decode_block.hip with one device array behind it: the LDS map's constants of every instantiation"""
    rows = ", ".join("B<%d, %s>::%s" % (rep, "true" if rvq else "false", f) for rep, rvq in PROBE_INSTANCES for f in PROBE_FIELDS)
    return ('#include "%s"\nnamespace quip {\ntemplate <int REP, bool RVQ> using B = BLds<REP, RVQ>;\n'
            'extern "C" __device__ __attribute__((used)) const int quip_lds_map_probe[] = {%s};\n}\n'
            % (os.path.join(CSRC, "decode_block.hip"), rows))


def _probe_values(asm):
    m = re.search(r"^quip_lds_map_probe:\n((?:\s+\.long\s+\S+.*\n)+)", asm, re.M)
    assert m, "the probe's array is not in the listing"
    vals = [int(x, 0) for x in re.findall(r"\.long\s+(\S+)", m.group(1))]
    assert len(vals) == len(PROBE_INSTANCES) * len(PROBE_FIELDS), len(vals)
    n = len(PROBE_FIELDS)
    return {inst: dict(zip(PROBE_FIELDS, vals[i * n:(i + 1) * n])) for i, inst in enumerate(PROBE_INSTANCES)}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_block_kernels_keep_their_resources_and_lose_the_barriers_the_design_removes(tmp_path):
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import check_inflight
    probe = tmp_path / "lds_map_probe.hip"
    probe.write_text(_probe_source())
    # (the probe IS decode_block.hip plus the array: its listing serves as that unit's)
    units = {"decode_block.hip": str(probe), "decode_block_g8.hip": "decode_block_g8.hip", "decode_block_tiled.hip": "decode_block_tiled.hip",
             "decode_block_gqa.hip": "decode_block_gqa.hip"}
    with ThreadPoolExecutor(max_workers=len(units)) as ex:
        built = dict(zip(units, ex.map(_compile, units.values())))

    # ---- the LDS map, as the compiler evaluated it ----
    maps = _probe_values(built["decode_block.hip"][0])
    for (rep, rvq), m in maps.items():
        print("BLds<%d, %d>:" % (rep, rvq), m)
        assert m["kBytes"] <= LDS_BUDGET and m["kBytes"] == m["kArea"] + m["kAreaBytes"], (rep, rvq, m)
        if rvq:
            assert m["kBuf1"] == m["kBuf0"], (rep, rvq, m)                    # no room: one buffer, every barrier
            continue
        end = m["kArea"] + m["kAreaBytes"]
        assert m["kBuf1"] == m["kBuf0"] + m["kBufBytes"] and m["kBuf1"] >= m["kArea"] + 3 * m["PSH"], (rep, m)
        assert m["kBuf1"] + 2 * m["kBufBytes"] <= end, (rep, m)               # two consumers: two rev buffers
        assert m["kHad"] >= m["kBuf1"] + m["kBufBytes"] and m["kStash"] >= m["kHad"] + 12032 and m["kStash"] + 6 * 1024 <= end, (rep, m)

    # ---- the kernels ----
    seen = set()
    for unit, (asm, remarks) in built.items():
        if unit == "decode_block_gqa.hip":
            kernels = [(n, l) for n, l in check_inflight.kernels_of(asm) if "decode_block_gqa_kernel" in n]
            assert len(kernels) == 1
            assert _barriers(kernels[0][1]) == PARENT_BARRIERS["gqa"], _barriers(kernels[0][1])     # fwd / rev defaults: what it was
            continue
        res = {n: f for n, f in _resources(remarks).items() if "decode_block_kernel" in n}
        kernels = [(n, l) for n, l in check_inflight.kernels_of(asm) if "decode_block_kernel" in n]
        assert kernels and sorted(res) == sorted(n for n, _ in kernels), (unit, sorted(res))
        assert len(kernels) == {"decode_block.hip": 7, "decode_block_g8.hip": 2, "decode_block_tiled.hip": 1}[unit]
        for name, lines in kernels:
            f = res[name]
            assert f["ScratchSize [bytes/lane]"] == 0, (unit, name, f)
            assert f["Occupancy [waves/SIMD]"] == 2, (unit, name, f)
            assert f["LDS Size [bytes/block]"] == 0, (unit, name, f)      # nothing static beside the dynamic BLds::kBytes checked above
            assert f["VGPRs"] <= (TILED_VGPRS if unit == "decode_block_tiled.hip" else 256), (unit, name, f)
            assert check_inflight.check_kernel(lines) == [], (unit, name)
            # <REP, RVQ, HI>: RVQ = true keeps ONE exchange buffer, and so does every kernel of the G8 unit
            kind = "g8" if unit == "decode_block_g8.hip" else ("rvq" if re.search(r"decode_block_kernelILi\d+ELb1E", name) else "two_buffers")
            seen.add(kind)
            want = PARENT_BARRIERS[kind] - (REMOVED if kind == "two_buffers" else 0)
            print(unit, name, kind, "s_barrier:", _barriers(lines), "parent:", PARENT_BARRIERS[kind], "VGPRs:", f["VGPRs"])
            assert _barriers(lines) == want, (unit, name, _barriers(lines), want)
    assert seen == {"two_buffers", "rvq", "g8"}
