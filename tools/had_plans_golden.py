#!/usr/bin/env python3
"""Writes tests/golden/had_plans.json: the launch plans of the Hadamard transforms (had_plan(), csrc/hadamard.hip) as the
library in the tree makes them through quip_had_plan(), for the cases of tests/test_had_plan_host.py.  No GPU is needed.
The file in the tree was recorded from launch_group() as it was before it was split into plan and launch
(profiles/had_host_refactor.txt) and tests/test_had_plan_host.py holds every later build to it.  Run this again only when
a plan is meant to change, and say in the commit which rows moved and what the kernels gained:
    python tools/had_plans_golden.py [out.json [name of the commit]]"""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from quip_for_all_amd import capi  # noqa: E402
from tests import test_had_plan_host as T  # noqa: E402


def _wrapped(items, width=150):
    """a JSON list, several items per line"""
    lines, cur = [], ""
    for it in (json.dumps(i, separators=(",", ":")) for i in items):
        if cur and len(cur) + len(it) + 1 > width:
            lines.append(cur)
            cur = ""
        cur += ("," if cur else "") + it
    return "[\n" + ",\n".join(lines + [cur]) + "\n]"


def write(out, head, plans):
    """plans: one per case of T.cases(), in the form of capi.had_plan()"""
    cs, e = T.cases(), T.encode(plans)
    assert len(plans) == len(cs)
    with open(out, "w") as f:
        f.write('{"recorded_on": %s,\n "cases": %d, "cases_sha256": "%s",\n "plan_fields": %s,\n "problem_fields": %s,\n "kinds": %s,\n'
                % (json.dumps(head or "unknown"), len(cs), T.cases_hash(cs), json.dumps(T.PLAN_FIELDS),
                   json.dumps(list(capi.HAD_PLAN_PROBLEM_FIELDS)), json.dumps(e["kinds"], indent=1)))
        f.write(' "problems": %s,\n "plans": %s,\n "rows": %s}\n' % (_wrapped(e["problems"]), _wrapped(e["plans"]), _wrapped(e["rows"])))
    print(len(plans), "plans,", len(e["plans"]), "distinct,", len(e["kinds"]), "kinds ->", out)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    head = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(["git", "rev-parse", "HEAD"], cwd=REPO, capture_output=True, text=True).stdout.strip()
    plans = [T.plan(c) for c in T.cases()]
    missing = sorted(set(capi.had_plan_kinds()) - {p[1] for p in plans})
    assert not missing, f"no case reaches {missing}: add one to cases()"
    write(out, head, plans)
