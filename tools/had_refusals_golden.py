#!/usr/bin/env python3
"""Writes tests/golden/had_refusals.json: what tests/test_had_boundary_host.py::test_every_refusal_is_the_recorded_one
compares with.  Per row of that module's table -- one Hadamard transform entry point of the C ABI on valid arguments
except for one or two faults -- the code the library answers.  No GPU is needed: every row is refused before any launch
or asks for no rows, and the recorder stops at the first row that is neither (that row is a mistake in the table).

Run it with QUIP_LIB_PATH pointing at the library of the commit whose answers are the reference -- the file in the tree was
recorded with the library of the parent of the commit that gave the transform launches one host path:
    QUIP_LIB_PATH=/path/to/parent/libquip_mi355.so python tools/had_refusals_golden.py [out.json [name of that commit]]"""
import ctypes
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from quip_for_all_amd import capi  # noqa: E402
from tests import test_had_boundary_host as T  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
lib = ctypes.CDLL(capi.LIB_PATH)      # (only the entries of the table: an older library need not have the newer symbols)
for entry in T.SPECS:
    getattr(lib, entry).argtypes = capi.SIGNATURES[entry]
rows = {}
for entry, faults in T.table():
    key = T.row_id(entry, faults)
    assert key not in rows, f"row named twice: {key}"
    code = T.call(lib, entry, faults)
    assert code in T.REFUSALS or (code == 0 and T.nothing_to_launch(faults)), \
        f"{key}: code {code} is no refusal -- the call reached a launch, the table is wrong"
    rows[key] = code
head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
names = {**T.REFUSALS, 0: "OK (no rows)"}
count = {name: sum(1 for c in rows.values() if c == code) for code, name in names.items()}
grouped = {}
for key, code in rows.items():
    entry, _, faults = key.partition(" ")
    grouped.setdefault(entry, {}).setdefault(str(code), []).append(faults)
with open(out, "w") as f:
    f.write('{"recorded_on": %s, "library": %s,\n "codes": %s,\n "rows": {\n' % (
        json.dumps(head or "unknown"), json.dumps(os.path.basename(os.environ.get("QUIP_LIB_PATH", "the tree's own"))),
        json.dumps({name: code for code, name in names.items()})))
    blocks = []
    for entry, by_code in grouped.items():
        parts = []
        for code, faults in sorted(by_code.items()):
            lines, cur = [], ""
            for it in map(json.dumps, faults):
                if cur and len(cur) + len(it) + 2 > 150:
                    lines.append(cur)
                    cur = ""
                cur += (", " if cur else "") + it
            parts.append('  "%s": [\n   %s]' % (code, ",\n   ".join(lines + [cur])))
        blocks.append(' "%s": {\n%s}' % (entry, ",\n".join(parts)))
    f.write(",\n".join(blocks) + "}}\n")
print("wrote", out, len(rows), "rows", count)
