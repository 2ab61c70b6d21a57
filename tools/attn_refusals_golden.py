#!/usr/bin/env python3
"""Writes tests/golden/attn_refusals.json: what tests/test_attn_boundary_host.py::test_every_refusal_is_the_recorded_one
compares with.  Per row of that module's table -- one attention entry point of the C ABI on valid arguments except for one
or two faults -- the code the library answers.  No GPU is needed: every row is refused before any launch, and the recorder
stops at the first row that is not (a code outside the four refusal codes: that row is a mistake in the table).

Run it with QUIP_LIB_PATH pointing at the library of the commit whose answers are the reference -- the file in the tree was
recorded with the library of the parent of the commit that gave the attention launches one host path:
    QUIP_LIB_PATH=/path/to/parent/libquip_mi355.so python tools/attn_refusals_golden.py [out.json [name of that commit]]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from quip_for_all_amd import capi  # noqa: E402
from tests import test_attn_boundary_host as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
lib = capi.lib()
rows = {}
for entry, faults in T.table():
    key = T.row_id(entry, faults)
    assert key not in rows, f"row named twice: {key}"
    code = T.call(lib, entry, faults)
    assert code in T.REFUSALS, f"{key}: code {code} is no refusal -- the call reached a launch, the table is wrong"
    rows[key] = code
head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
count = {name: sum(1 for c in rows.values() if c == code) for code, name in T.REFUSALS.items()}
with open(out, "w") as f:
    json.dump({"recorded_on": head or "unknown", "library": os.path.basename(os.environ.get("QUIP_LIB_PATH", "the tree's own")),
               "codes": {name: code for code, name in T.REFUSALS.items()}, "rows": rows}, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", out, len(rows), "rows", count)
