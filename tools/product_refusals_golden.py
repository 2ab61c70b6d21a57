#!/usr/bin/env python3
"""Writes tests/golden/product_refusals.json: what tests/test_product_boundary_host.py::test_every_answer_is_the_recorded_one
compares with.  Per row of that module's table -- one product entry point of the C ABI on valid arguments except for one or
two faults -- the code the library answers.  No GPU is needed: every row is answered before any launch, and the recorder
stops at the first row that is not (a code outside the four refusal codes and QUIP_OK, QUIP_ERR_LAUNCH above all: that row
is a mistake in the table), and at a QUIP_OK in a row that has no empty dimension.

Run it with QUIP_LIB_PATH pointing at the library of the commit whose answers are the reference -- the file in the tree was
recorded with the library of the parent of the commit that gave the product launches one host path -- and with QUIP_GEMV_V2
and QUIP_GEMV_NIB unset:
    QUIP_LIB_PATH=/path/to/parent/libquip_mi355.so python tools/product_refusals_golden.py [out.json [name of that commit]]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from quip_for_all_amd import capi  # noqa: E402
from tests import test_product_boundary_host as T  # noqa: E402

assert "QUIP_GEMV_V2" not in os.environ and "QUIP_GEMV_NIB" not in os.environ, "the planner's switches change the answers"
out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
lib = capi.lib()
rows = {}
for entry, faults in T.table():
    key = T.row_id(entry, faults)
    assert key not in rows, f"row named twice: {key}"
    code = T.call(lib, entry, faults)
    assert code in T.ANSWERS, f"{key}: code {code} is no answer before a launch -- the table is wrong"
    assert code != 0 or any(faults.get(e) == 0 for e in T.EMPTY), f"{key}: QUIP_OK without an empty dimension"
    rows[key] = code
head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
count = {name: sum(1 for c in rows.values() if c == code) for code, name in T.ANSWERS.items()}
assert all(count.values()), f"an answer never occurs: {count}"
by_entry = {}
for key, code in rows.items():
    entry, faults = key.split(" ", 1)
    by_entry.setdefault(entry, {})[faults] = code
with open(out, "w") as f:
    json.dump({"recorded_on": head or "unknown", "library": os.path.basename(os.environ.get("QUIP_LIB_PATH", "the tree's own")),
               "codes": {name: code for code, name in T.ANSWERS.items()}, "rows": by_entry}, f, indent=0, sort_keys=True)
    f.write("\n")
print("wrote", out, len(rows), "rows", count)
