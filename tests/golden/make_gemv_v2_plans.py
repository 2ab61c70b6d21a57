"""Writes tests/golden/gemv_v2_plans.json: the launch plans of the K-splitting GEMV (csrc/e8p_gemv_v2_plan.hip.h) as the
library in the tree makes them, through the quip_e8p_gemv_v2_plan hook.  The file was recorded from the planners as they
were before they were split into plan + launch; tests/test_launch_layer_host.py holds every later build to it.  Run this
again only when a plan is meant to change, and say in the commit which rows moved and what the kernels gained."""
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)

SHAPES = [    # (ns, k, blocks)
    ([4096], 4096, 0), ([11008, 11008], 4096, 0), ([4096], 11008, 0), ([8192], 8192, 0), ([8192, 1024, 1024], 8192, 0),
    ([28672], 8192, 0), ([28672, 28672], 8192, 0), ([8192], 28672, 0), ([8192], 57344, 0), ([1], 128, 0), ([5], 128, 0),
    ([4], 1024, 0), ([4096], 4096, 1),     # blocks = 1: the row-block doubling loop
]
COLUMNS = ["ns", "k", "rep", "slots", "blocks", "ksplit", "max_waves", "runlen", "grid2", "ws", "plan"]


def cases():
    for ns, k, blocks in SHAPES:
        for ws in (1, 0):
            for rep in (0, 32, 24, 16, 64, 4):
                yield (ns, k, rep, 0, blocks, 0, 0, 0, 0, ws)
            if len(ns) == 1:                      # E8P12RVQ3B: one problem, needs its second table
                for g2 in (1, 0):
                    yield (ns, k, 40, 0, blocks, 0, 0, 0, g2, ws)
        for rep in (0, 4):
            for slots in (1, 3, 4):
                yield (ns, k, rep, slots, blocks, 0, 0, 0, 0, 1)
            yield (ns, k, rep, 0, blocks, 2, 0, 0, 0, 1)      # forced K split
            yield (ns, k, rep, 0, blocks, 2, 0, 0, 0, 0)      # ... without a workspace
            yield (ns, k, rep, 0, blocks, 0, 0, 1, 0, 1)      # forced run length
            for mw in (8, 16):
                yield (ns, k, rep, 0, blocks, 0, mw, 0, 0, 1)
    yield ([4096, 4096, 4096, 4096], 4096, 0, 0, 0, 0, 0, 0, 0, 1)      # count > 3
    yield ([4096], 4100, 0, 0, 0, 0, 0, 0, 0, 1)                        # k % 128


def record():
    from quip_for_all_amd import capi
    rows = []
    for ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws in cases():
        plan = capi.gemv_v2_plan(ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws)
        rows.append([ns, k, rep, slots, blocks, ksplit, mw, runlen, g2, ws, plan])
    return rows


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", "gemv_v2_plans.json")
    rows = record()
    with open(out, "w") as f:
        f.write('{"columns": %s,\n "plan_fields": %s,\n "rows": [\n' % (json.dumps(COLUMNS), json.dumps(
            ["rc", "rep", "slots", "ksplit", "nrb", "spw", "rpb0", "rpb1", "rpb2", "runlen", "rpr_inv", "threads", "lds"])))
        f.write(",\n".join("  " + json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(len(rows), "plans ->", out)
