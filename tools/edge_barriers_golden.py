#!/usr/bin/env python3
"""Writes tests/golden/edge_barriers/golden.json: what tests/test_gpu_edge_barriers.py::test_same_bits_as_before_the_change compares
with.  Per changed instantiation of the persistent block launch (launch-tiled E8P12, row-major nibble E8P12, D4), for 1 and 2 blocks,
from position 0 and from position 100 behind a fixed history: six greedy steps from token 7 -- per step sha256 of the fp16 logits, the
next token and 16 sampled logits (fp16 bit patterns); sha256 of the appended K / V cache rows; a sha256 of the blocks' Qidxs / SU / SV
as a fingerprint of the inputs.

Run it with QUIP_LIB_PATH pointing at the library of the commit whose results are the reference -- the file in the tree was recorded
with the library of the parent of the commit that gave the 4096-wide edges their second exchange buffer:
    QUIP_LIB_PATH=/path/to/parent/libquip_mi355.so python tools/edge_barriers_golden.py [out.json [name of that commit]]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import test_gpu_edge_barriers as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
cases = {}
for build in T.BUILDS:
    for layers in (1, 2):
        for pos0 in T.POSITIONS:
            key = f"{build}-{layers}-{pos0}"
            cases[key] = T.measure(build, layers, pos0)
            print(key, cases[key]["steps"][-1]["logits_sha256"][:16], [s["token"] for s in cases[key]["steps"]], flush=True)
head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_on": head or "unknown", "library": os.path.basename(os.environ.get("QUIP_LIB_PATH", "the tree's own")),
               "steps": T.STEPS, "first_token": T.TOKEN, "positions": T.POSITIONS, "sampled_logits": T.SAMPLED, "cases": cases},
              f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out)
