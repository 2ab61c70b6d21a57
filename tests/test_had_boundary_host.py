"""What the Hadamard transform entry points of the C ABI refuse, and with which code, without a GPU: the seven
quip_had_transform_* calls and quip_hadamard_f16 against tests/golden/had_refusals.json, recorded by
tools/had_refusals_golden.py from the library of the commit before the transform launches got one host path.  Every row
is refused before any launch, or asks for no rows at all (NULL stream, host scratch for every pointer), so the comparison
is code for code: which pointers an entry looks at, which alignment it asks of each, and which code wins where two things
are wrong at once."""
import ctypes
import json
import os

import pytest

from quip_for_all_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "had_refusals.json")
REFUSALS = {-1: "NULL_POINTER", -2: "BAD_SHAPE", -3: "MISALIGNED", -5: "UNSUPPORTED"}

# An entry's arguments in the order of include/quip_mi355.h: a bare name is a pointer, name=V a number with a valid value,
# `fusion` a quip_had_fusion (its pointers: fusion.residual, ...), `problems` an array of `count` quip_had_problem (their
# fields: p0.x, p1.out, ...), stream always NULL.  1408 = 11 x 128: K > 1, so a NULL `had` is refused by itself.
_F16 = "x y rows=3 in_features=1400 out_features=1400 n=1408 K=11 had transpose=0 pre_scale pre_scale2 post_scale bias scale=1.0"
_PLANES = "x planes in_features=1400 n=1408 K=11 had transpose=1 pre_scale scale=1.0"
SPECS = {
    "quip_hadamard_f16": "x y rows=3 n=1024 scale=1.0 stream",
    "quip_had_transform_f16": _F16 + " stream",
    "quip_had_transform_planes": _PLANES + " stream",
    "quip_had_transform_fused_f16": _F16 + " fusion stream",
    "quip_had_transform_planes_fused": _PLANES + " fusion stream",
    "quip_had_transform_group_f16": "problems count=2 rows=3 n=1408 K=11 transpose=0 stream",
    "quip_had_transform_planes_group": "problems count=2 n=1408 K=11 transpose=1 stream",
    "quip_had_transform_planes_rows": "problems rows=3 n=1408 K=11 transpose=1 stream",
}
FUSION_PTRS = ("residual", "rms_weight", "gate")
PROBLEM_PTRS = ("x", "out", "had", "pre_scale", "pre_scale2", "post_scale", "bias", "residual", "rms_weight", "gate")
CHAIN_PTRS = ("z", "z_post_scale", "z_residual", "h_out", "z_had")
ANCHOR = {"n": 3}            # a size every entry answers BAD_SHAPE: beside it, a fault that alone is no refusal still shows

_buf = (ctypes.c_char * 8192)()
P16 = ((ctypes.addressof(_buf) + 15) & ~15) + 256
_SLOT = {name: P16 + 64 * i for i, name in enumerate(("x", "y", "planes", "out") + PROBLEM_PTRS[2:] + CHAIN_PTRS)}


def _at(name, faults, key):
    """the pointer `name` under the fault at `key`: absent -> valid, None -> NULL, a number -> off by that many bytes,
    "=other" -> the address of `other`"""
    if key not in faults:
        return _SLOT[name]
    f = faults[key]
    return None if f is None else _SLOT[f[1:]] if isinstance(f, str) else _SLOT[name] + f


def call(lib, entry, faults):
    """`entry` on valid arguments except at `faults`, {argument or field: value}.  `chain` (problem-struct entries): every
    problem is a chain on z / z_post_scale / z_residual / h_out / z_had with in_features = n and no x."""
    planes = "planes" in entry
    num = {t.split("=")[0]: t.split("=")[1] for t in SPECS[entry].split() if "=" in t}
    num = {k: faults.get(k, float(v) if k == "scale" else int(v)) for k, v in num.items()}
    keep, args = [], []
    for tok in SPECS[entry].split():
        name = tok.split("=")[0]
        if name == "stream":
            args.append(None)
        elif "=" in tok:
            args.append(num[name])
        elif name == "fusion":
            if faults.get("fusion", 0) is None:
                args.append(None)
                continue
            f = capi.HadFusion(*[_at(p, faults, "fusion." + p) for p in FUSION_PTRS], 1e-5)
            keep.append(f)
            args.append(ctypes.addressof(f))
        elif name == "problems":
            chain = faults.get("chain", 0)
            count = max(1, min(int(num.get("count", 1)), 3))
            arr = (capi.HadProblem * 3)()
            for i in range(count):
                pr, pre = arr[i], f"p{i}."
                for p in PROBLEM_PTRS:
                    setattr(pr, p, _at(p, faults, pre + p))
                pr.in_features = faults.get(pre + "in_features", num["n"] if chain else 1400)
                pr.out_features = faults.get(pre + "out_features", num["n"] if planes or chain else 1400)
                pr.scale, pr.rms_eps, pr.z_scale = 1.0, 1e-5, 1.0
                for k in ("resid_scale", "planes_layout", "n"):
                    setattr(pr, k, faults.get(pre + k, 0))
                if chain:
                    pr.x = pr.gate = pr.pre_scale2 = None
                    for p in CHAIN_PTRS:
                        setattr(pr, p, _at(p, faults, pre + p))
                    for p in ("x", "gate", "pre_scale2"):     # (not part of a valid K > 1 chain: only as a fault)
                        if pre + p in faults:
                            setattr(pr, p, _at(p, faults, pre + p))
            keep.append(arr)
            args.append(None if faults.get("problems", 0) is None else ctypes.addressof(arr))
        else:
            args.append(_at(name, faults, name))
    return getattr(lib, entry)(*args)


def row_id(entry, faults):
    return entry + " " + " ".join(f"{k}={faults[k]}" for k in sorted(faults))


def recorded(golden):
    """{row_id: code} of the file, which groups the rows as {entry: {code: [the faults of a row, ...]}}"""
    return {entry + " " + faults: int(code) for entry, by_code in golden["rows"].items() for code, rows in by_code.items()
            for faults in rows}


def nothing_to_launch(faults):
    return faults.get("rows", 1) <= 0


def table():
    """[(entry, faults)]: every row a call that is refused before any launch, or one of no rows"""
    rows = []
    for entry in SPECS:
        toks = SPECS[entry].split()
        put = lambda f: (entry, dict(f)) in rows or rows.append((entry, dict(f)))  # noqa: E731  (one problem: some rows coincide)
        struct, planes = "problems" in toks, "planes" in entry
        count = 1 if entry.endswith("_rows") else 2
        ptrs = [t for t in toks if "=" not in t and t not in ("stream", "fusion", "problems")]
        if "fusion" in toks:
            ptrs += ["fusion"] + ["fusion." + p for p in FUSION_PTRS]
        if struct:
            ptrs += ["problems"] + [f"p{i}.{p}" for i in range(count) for p in PROBLEM_PTRS]
        # every pointer NULL, alone and beside the anchor
        for p in ptrs:
            alone = p in ("x", "y", "planes", "had", "problems") or p.endswith((".x", ".out", ".had"))
            if alone:
                put({p: None})
            put({p: None, **ANCHOR})
        # every pointer off by 2, 4 and 8: alone where that is refused (plane images), and beside the anchor
        for p in ptrs:
            if p in ("fusion", "problems"):
                continue
            for d in (2, 4, 8):
                if p == "planes" or (planes and p.endswith(".out")):
                    put({p: d})
                put({p: d, **ANCHOR})
        # sizes at their limits
        if entry == "quip_hadamard_f16":
            for n in (0, 3, 1000, 65536):
                put({"n": n})
        else:
            put({"K": 0})
            put({"K": -1})
            put({"n": 1409})                      # n % K
            put({"n": 11 * 96})                   # L not a power of two
            put({"n": 11 * 65536})                # L > 32768
            put({"n": 0})
            feats = ("in_features",) if planes else ("in_features", "out_features")
            for f in ([f"p{i}.{f}" for i in range(count) for f in feats] if struct else feats):
                put({f: 0})
                put({f: 1409})
                put({f: -1})
        if "count=2" in toks:
            for c in (0, 4, -1):
                put({"count": c})
        if "rows=3" in toks:
            for r in (-1, 0):
                put({"rows": r})
                put({"rows": r, **ANCHOR})
                put({"rows": r, ptrs[0]: None})
                if entry != "quip_hadamard_f16":
                    put({"rows": r, "had": None} if not struct else {"rows": r, "p0.had": None})
        # two faults of different classes: which code wins
        if planes and not struct:
            put({"planes": 2, "x": None})
            put({"planes": 2, "had": None})
            put({"planes": 2, "K": 0})
        if not struct and entry != "quip_hadamard_f16":
            put({"had": None, "K": 0})
            put({"had": None, "in_features": 0})
            put({"x": None, "K": 0})
        if struct:
            last = count - 1
            put({"problems": None, "count": 0})
            put({f"p{last}.x": None, "K": 0})               # every problem's x / out before any size
            put({f"p{last}.out": None, "p0.in_features": 0})
            put({f"p{last}.had": None, "p0.in_features": 0})   # ... the rest problem by problem
            put({"p0.had": None, f"p{last}.in_features": 0})
            if planes:
                put({f"p{last}.out": 4, "p0.in_features": 0})
                put({"p0.out": 4, f"p{last}.in_features": 0})
                put({"p0.out": 4, "p0.had": None})
                put({"p0.planes_layout": 3})
                put({"p0.planes_layout": -1})
                put({"p0.planes_layout": 3, "p0.out": 4})
                put({"p0.planes_layout": 3, "p0.in_features": 0})
                put({"n": 44, "K": 11})                       # n % 16
                put({"n": 8, "K": 4, "p0.in_features": 8, "p1.in_features": 8})       # L < 4
                for rs, lay in ((0.5, 0), (0.0, 2)):          # the virtual-vector layouts: blocked kernels only
                    put({"n": 128, "K": 1, "p0.resid_scale": rs, "p0.planes_layout": lay, "p0.in_features": 128, "p1.in_features": 128})
                    put({"n": 352, "K": 11, "p0.resid_scale": rs, "p0.planes_layout": lay, "p0.in_features": 352, "p1.in_features": 352})
            # a problem of its own width: fp16, K == 1, no rms_weight, no chain, 256 <= width <= 16384
            put({"p0.n": 2816})
            put({"p0.n": 2816, "K": 0})
            k1 = {"n": 1024, "K": 1, "p0.in_features": 1024, "p0.out_features": 1024}
            if not planes:
                k1.update({"p1.in_features": 1024, "p1.out_features": 1024})
            put({**k1, "p0.n": 2048})                         # (fp16: rms_weight is there)
            if not planes:
                put({**k1, "p0.n": 2048, "p0.rms_weight": None, "p1.rms_weight": None, "p0.in_features": 4096})
                put({**k1, "p0.n": 128, "p0.rms_weight": None, "p1.rms_weight": None, "p0.in_features": 100, "p0.out_features": 100})
                put({**k1, "p0.n": 32768, "p0.rms_weight": None, "p1.rms_weight": None})
                put({**k1, "p0.n": 3000, "p0.rms_weight": None, "p1.rms_weight": None})
            # every chain condition
            c5 = {"chain": 1, "n": 5120, "K": 5}
            c1 = {"chain": 1, "n": 4096, "K": 1}
            for c in (c5, c1):
                k = c["K"]
                put({**c, "p0.in_features": c["n"] - 8})
                put({**c, "p0.z_post_scale": None})
                put({**c, "p0.h_out": None})
                put({**c, f"p{last}.h_out": None})
                put({**c, "p0.z_had": None} if k > 1 else {**c, "p0.z_had": None, "p0.z": 2})      # (K == 1 does not look)
                put({**c, "p0.h_out": "=z_residual"})
                put({**c, "p0.h_out": "=z"} if k > 1 and planes else {**c, "p0.h_out": "=z", "p0.z": 2})
                for p in ("z", "z_post_scale", "z_residual", "h_out"):
                    for d in (2, 4, 8):
                        put({**c, "p0." + p: d})
                for p in ("pre_scale", "rms_weight", "z_had", "had"):
                    put({**c, "p0." + p: 2} if k > 1 and planes and p in ("pre_scale", "rms_weight") else {**c, "p0." + p: 2, "p0.z": 2})
                put({**c, "p0.z": 2, "p0.z_post_scale": None})      # NULL before MISALIGNED before the aliases
                put({**c, "p0.z": 2, "p0.h_out": "=z_residual"})
                put({**c, "p0.z_post_scale": None, "p0.in_features": c["n"] - 8})
                if planes:
                    put({**c, "p0.out": 4})
                    put({**c, "p0.out": 4, "p0.z": 2})
                if entry.endswith("_rows"):
                    put({**c, "rows": 2} if k > 1 else {**c, "rows": 2, "p0.z": 2})
                    put({**c, "rows": 0})
                    put({**c, "rows": -1})
                if count > 1 and k > 1:
                    put({**c, "p1.z": None, "p1.x": 0})              # a launch is all chain or no chain
                put({**c, "p0.z": None, "p0.x": None})
            put({**c5, "p0.gate": 0})
            put({**c5, "p0.pre_scale2": 0})
            put({"chain": 1, "n": 128, "K": 1})
            put({"chain": 1, "n": 32768, "K": 1})
            for n, K in ((6 * 1024, 6), (9 * 512, 9), (3 * 256, 3), (3 * 8192, 3), (5 * 4096, 5), (5120, 20), (11008, 43)):
                put({"chain": 1, "n": n, "K": K})
            put({**c1, "p0.n": 2048})
    return rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    return capi.lib()


def test_the_table_covers_every_transform_entry_and_names_each_row_once():
    want = {n for n in capi.SIGNATURES if n.startswith("quip_had_transform_")} | {"quip_hadamard_f16"}
    assert set(SPECS) == want and len(want) == 8
    for entry in SPECS:
        assert len(SPECS[entry].split()) == len(capi.SIGNATURES[entry]), entry
    ids = [row_id(*r) for r in table()]
    assert len(ids) == len(set(ids))


def test_every_refusal_is_the_recorded_one(lib):
    with open(GOLDEN) as f:
        golden = json.load(f)
    rows, answers = table(), recorded(golden)
    assert sorted(answers) == sorted(row_id(*r) for r in rows)
    wrong = {}
    for entry, faults in rows:
        key = row_id(entry, faults)
        want = answers[key]
        assert want in REFUSALS or (want == 0 and nothing_to_launch(faults)), key     # (never a call that could launch)
        got = call(lib, entry, faults)
        if got != want:
            wrong[key] = (want, got)
    assert not wrong, f"{len(wrong)} of {len(rows)} answers moved: {dict(list(wrong.items())[:8])}"
