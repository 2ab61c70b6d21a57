"""The launch plans of the Hadamard transforms (had_plan() in csrc/hadamard.hip) against tests/golden/had_plans.json,
without a GPU.  The transforms agree across kernel instantiations bit for bit, so a shape that lands on another
instantiation, grid or LDS size shows in no result: the table pins which instantiation serves which group, on what grid,
and the per-launch fields of the kernel arguments, field for field.  It was recorded from launch_group() as it was before
it was split into plan and launch (profiles/had_host_refactor.txt); tools/had_plans_golden.py regenerates it through
quip_had_plan().  Pointers are host scratch: the hook looks at NULL and alignment and never dereferences.

The file holds no case list: cases() below is the list (the file carries its length and hash), and the plans stand in
its order as indices into the distinct plans, whose per-problem fields are indices into the distinct sextuples."""
import ctypes
import hashlib
import json
import os

import pytest

from quip_for_all_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "had_plans.json")
PLAN_FIELDS = ["rc", "kind", "grid_x", "grid_y", "grid_z", "threads", "lds", "then one index into `problems` per problem"]

KS = (1, 3, 5, 7, 11, 20, 28, 43, 172)
LS = tuple(1 << e for e in range(2, 16))             # 4 .. 32768
ROWS = (1, 8, 9, 31, 32, 33)
# where the element-wise vectors, the groups and the alignment decide: the tall shapes of every length with few and many
# row tiles, the blocked ones with K = 1 and with a small odd K
SOME = [(K, K * L) for K in (3, 43, 172) for L in (64, 128, 256)] + [(K, K * L) for K in (1, 7, 11) for L in (1024, 4096)] + [(1, 8192)]
# optional vectors of a problem, one letter each
VECTORS = {"p": "pre_scale", "2": "pre_scale2", "g": "gate", "r": "rms_weight", "o": "post_scale", "b": "bias", "s": "residual"}
_SLOTS = ("x", "out", "had", "pre_scale", "pre_scale2", "post_scale", "bias", "residual", "rms_weight", "gate", "z",
          "z_post_scale", "z_residual", "h_out", "z_had")
_buf = (ctypes.c_char * 8192)()
P16 = ((ctypes.addressof(_buf) + 15) & ~15) + 256


def cases():
    """(planes, K, ns, rows, chain, vectors, off, din, dout): ns the problems' widths (the launch's n is ns[0]), chain 0 /
    1 (with z_residual) / 2 (without), vectors one string of VECTORS' letters per problem, off {field: bytes} moves
    pointers of the last problem, din / dout: in_features = n - din, out_features = n - dout"""
    out = []
    put = lambda *c: out.append(c)  # noqa: E731
    # every shape, plain
    for K in KS:
        for L in LS:
            for rows in ROWS:
                for planes in (0, 1):
                    put(planes, K, [K * L], rows, 0, [""], {}, 0, 0)
    for K, n in SOME:
        for rows in (1, 9, 32):
            # fp16: each optional vector, the two sides together; in a group the last problem carries them
            for v in ("p", "2", "g", "r", "o", "b", "s", "po", "gs"):
                put(0, K, [n], rows, 0, [v], {}, 0, 0)
            for count in (2, 3):
                for v in ("", "p", "o", "po", "r"):
                    put(0, K, [n] * count, rows, 0, [""] * (count - 1) + [v], {}, 0, 0)
            # operands off 16-byte alignment, sizes off the 8-chunks
            for v, off in (("", {"x": 2}), ("", {"out": 2}), ("p", {"pre_scale": 2}), ("o", {"post_scale": 8}),
                           ("s", {"residual": 4}), ("g", {"gate": 2})):
                put(0, K, [n], rows, 0, [v], off, 0, 0)
            put(0, K, [n], rows, 0, [""], {}, 0, 4)
            put(0, K, [n], rows, 0, [""], {}, 4, 0)
            put(0, K, [n, n], rows, 0, ["", ""], {}, 0, 4)
        # planes: groups of one row, single problems of several rows
        for count in (1, 2, 3):
            for v in ("", "p", "r", "g"):
                put(1, K, [n] * count, 1, 0, [""] * (count - 1) + [v], {}, 0, 0)
        for rows in (9, 32):
            for v in ("p", "r", "g"):
                put(1, K, [n], rows, 0, [v], {}, 0, 0)
        put(1, K, [n], 1, 0, [""], {"x": 2}, 0, 0)
        put(1, K, [n], 1, 0, [""], {}, 4, 0)
    # K == 1 fp16 groups of mixed widths (q next to the narrower k / v of a grouped-query model)
    for ns in ([4096, 1024, 1024], [8192, 1024, 1024], [1024, 4096], [256, 16384], [16384, 256, 512], [4096, 512], [512, 512, 256]):
        for rows in ROWS:
            for v in ("", "o"):
                put(0, 1, ns, rows, 0, [""] * (len(ns) - 1) + [v], {}, 0, 0)
    # chains.  K == 1: both kinds, 256 <= n <= 16384
    for n in (256, 1024, 4096, 8192, 16384):
        for count in (1, 2, 3):
            for v in ("", "r", "p"):
                put(1, 1, [n] * count, 1, 1, [v] * count, {}, 0, 0)
                for rows in (1, 32):
                    put(0, 1, [n] * count, rows, 1, [v] * count, {}, 0, 0)
    # K in {3, 5, 7}: the planes group, one row (n > 16384 answers UNSUPPORTED)
    for K in (3, 5, 7):
        for L in (512, 1024, 2048, 4096):
            for count in (1, 3):
                for v in ("", "r", "p"):
                    for chain in (1, 2):
                        put(1, K, [K * L] * count, 1, chain, [v] * count, {}, 0, 0)
    return out


def problems(case):
    planes, K, ns, rows, chain, vectors, off, din, dout = case
    prs = []
    for i, n in enumerate(ns):
        at = {name: P16 + 64 * j for j, name in enumerate(_SLOTS)}
        if i == len(ns) - 1:
            at = {name: p + off.get(name, 0) for name, p in at.items()}
        pr = capi.HadProblem()
        pr.x, pr.out, pr.had = None if chain else at["x"], at["out"], at["had"] if K > 1 else None
        for letter in vectors[i]:
            setattr(pr, VECTORS[letter], at[VECTORS[letter]])
        pr.in_features, pr.out_features = n - din, n - dout
        pr.scale, pr.rms_eps, pr.z_scale = 1.0, 1e-5, 1.0
        if chain:
            pr.z, pr.z_post_scale, pr.h_out = at["z"], at["z_post_scale"], at["h_out"]
            pr.z_residual = at["z_residual"] if chain == 1 else None
            pr.z_had = at["z_had"] if K > 1 else None
        pr.n = n if len(set(ns)) > 1 else 0
        prs.append(pr)
    return prs


def plan(case):
    planes, K, ns, rows = case[:4]
    return capi.had_plan(problems(case), planes, rows, ns[0], K, 1 if planes else 0)


def cases_hash(cs):
    return hashlib.sha256(json.dumps([list(c) for c in cs], separators=(",", ":")).encode()).hexdigest()


def encode(plans):
    """the plans of cases(), as capi.had_plan() gives them, in the file's form"""
    kinds, problems, distinct, rows = [], [], [], []
    index = lambda seq, v: seq.index(v) if v in seq else (seq.append(v) or len(seq) - 1)  # noqa: E731
    for plan in plans:
        head = [plan[0], None if plan[1] is None else index(kinds, plan[1])] + list(plan[2:7])
        rows.append(index(distinct, head + [index(problems, list(p)) for p in plan[7:]]))
    return {"kinds": kinds, "problems": problems, "plans": distinct, "rows": rows}


def decode(golden):
    """[plan of every case], in the form of capi.had_plan()"""
    out = []
    for i in golden["rows"]:
        p = golden["plans"][i]
        out.append([p[0], None if p[1] is None else golden["kinds"][p[1]]] + p[2:7] + [golden["problems"][j] for j in p[7:]])
    return out


@pytest.fixture(scope="module")
def golden():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_is_the_case_list(golden):
    cs = cases()
    assert golden["cases"] == len(cs) == len(golden["rows"]) and golden["cases_sha256"] == cases_hash(cs)


def test_every_plan_is_the_recorded_one(golden):
    cs = cases()
    wrong = [(c, want, plan(c)) for c, want in zip(cs, decode(golden)) if plan(c) != want]
    assert not wrong, f"{len(wrong)} of {len(cs)} plans moved, first: {wrong[0]}"


def test_every_plan_kind_is_in_the_table(golden):
    seen = {p[1] for p in decode(golden)} - {None}
    kinds = capi.had_plan_kinds()
    assert len(kinds) == len(set(kinds)) == 40
    assert seen == set(kinds), sorted(set(kinds) - seen)


def test_the_hook_refuses_what_the_entry_points_refuse():
    NULL, BAD_SHAPE, UNSUPPORTED = -1, -2, -5
    lib = capi.lib()
    out = (ctypes.c_int32 * 25)()
    ok = problems((0, 1, [4096], 1, 0, [""], {}, 0, 0))
    arr = (capi.HadProblem * 1)(*ok)
    assert lib.quip_had_plan(arr, 1, 0, 1, 4096, 1, 0, None) == NULL
    assert lib.quip_had_plan(None, 1, 0, 1, 4096, 1, 0, out) == NULL and list(out)[:2] == [NULL, -1]
    assert lib.quip_had_plan(arr, 4, 0, 1, 4096, 1, 0, out) == BAD_SHAPE
    assert lib.quip_had_plan(arr, 1, 0, 1, 4097, 1, 0, out) == BAD_SHAPE and list(out)[:2] == [BAD_SHAPE, -1]
    assert capi.had_plan(problems((1, 5, [5 * 8192], 1, 1, [""], {}, 0, 0)), 1, 1, 5 * 8192, 5, 1) == [UNSUPPORTED, None, 0, 0, 0, 0, 0]
    # nothing to launch: validated, no plan
    assert capi.had_plan(ok, 0, 0, 4096, 1) == [0, None, 0, 0, 0, 0, 0]
    # a batch longer than grid.y goes out in slices: the plan is the first slice's
    assert capi.had_plan(ok, 0, 70000, 4096, 1)[:5] == [0, "had_kone_batch_kernel<12>", 1, 65535, 1]
