#!/usr/bin/env python3
"""Writes tests/golden/mlp_rows/golden.json: what tests/test_gpu_mlp_rows.py::test_same_bits_as_before_the_change compares with.
Per instantiation of the persistent block launch and for 1 and 2 blocks: six greedy steps from token 7, then sha256 of the logits and
of the new K / V cache rows of the sixth step, the next token, the first 16 logits (fp16 bit patterns) and a sha256 of the blocks'
Qidxs / SU / SV as a fingerprint of the inputs.

Run it on the commit whose results are the reference -- the file in the tree was recorded on the parent of the commit that moved the
row owners of the MLP edge onto one wave per row -- or with QUIP_LIB_PATH pointing at that commit's library:
    python tools/mlp_rows_golden.py [out.json [name of the commit, where git cannot tell]]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from tests import test_gpu_mlp_rows as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
cases = {}
for build in T.BUILDS:
    for layers in (1, 2):
        cases[f"{build}-{layers}"] = T.measure(build, layers)
        print(build, layers, cases[f"{build}-{layers}"]["logits_sha256"][:16], cases[f"{build}-{layers}"]["token"], flush=True)
head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
with open(out, "w") as f:
    json.dump({"recorded_on": head or "unknown", "library": os.path.basename(os.environ.get("QUIP_LIB_PATH", "the tree's own")),
               "steps": T.STEPS, "first_token": T.TOKEN, "cases": cases}, f, indent=1, sort_keys=True)
    f.write("\n")
print("wrote", out)
