"""What the product entry points of the C ABI answer before any launch, and with which code, without a GPU: the stand-alone
GEMVs, rows mode, the original-order, skinny and batched products and decompress against
tests/golden/product_refusals.json, recorded by tools/product_refusals_golden.py from the library of the commit before the
product host path was unified.  Every row is answered before any launch (NULL stream, host scratch for every pointer), so
the comparison is code for code: which pointers an entry looks at, which alignment it asks of each, and which answer wins
where two things are wrong at once.  The accepted empty calls (m, n or rows of 0: QUIP_OK, no launch) are rows too: where
an entry answers them among its other checks is what differs from entry to entry.  QUIP_GEMV_V2 / QUIP_GEMV_NIB stay unset."""
import ctypes
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "product_refusals.json")
ANSWERS = {0: "OK", -1: "NULL_POINTER", -2: "BAD_SHAPE", -3: "MISALIGNED", -5: "UNSUPPORTED"}
EMPTY = ("m", "rows", "n")          # QUIP_OK is a legal answer only in a row that has one of these at 0

# An entry's arguments in the order of include/quip_mi355.h.  name:A -- a pointer the entry (or the launcher behind it, before
# the launch) wants A-byte aligned (1: nobody looks); name:?A -- an optional pointer (NULL is a legal value: no NULL row);
# name:gA -- a host array of `count` device pointers (elements name[i]); ns:n -- the host int32 array of the problems' n;
# in:f -- quip_gemv_fused_in; name=V -- a number with a valid value; stream -- always NULL.
_ONE = "planes:16 qidxs:16 grid:64 y:1 n=256 k=4096"
_GRP = "planes:g16 qidxs:g{q} grid:64 {g2}ys:g1 ns:n count=2 k=4096"
_WS = " workspace:?16 ws_bytes=1048576 stream"
_MM = "x:16 qidxs:1 {t}y:1 m=2 n=256 k=4096 stream"
_SK = "x:16 qidxs:{q} {t}y:4 m=4 n=256 k=4096 stream"
_BA = "x:16 qidxs:16 {t}y:16 m=64 n=256 k=4096 stream"
_DEC = "qidxs:1 {t}w:16 rows=4 k=4096 stream"
_T1, _T = "grid:{a} ", "grid:{a} scale=0.5 "
SPECS = {
    "quip_e8p_gemv_planes": _ONE + " stream",
    "quip_e8p_gemv_planes_ws": _ONE + _WS,
    "quip_e8p_gemv_planes_group": _GRP.format(q=16, g2="") + " stream",
    "quip_e8p_gemv_planes_group_ws": _GRP.format(q=16, g2="") + _WS,
    "quip_d4_gemv_planes_group": _GRP.format(q=16, g2="") + " stream",
    "quip_d4_gemv_planes_group_ws": _GRP.format(q=16, g2="") + _WS,
    "quip_e8prvq3_gemv_planes_group": _GRP.format(q=4, g2="grid2:8 ") + " stream",
    "quip_e8prvq3_gemv_planes_group_ws": _GRP.format(q=4, g2="grid2:8 ") + _WS,
    "quip_d4_gemv_planes": _ONE + " stream",
    "quip_d4_gemv_planes_v2": _ONE + _WS,
    "quip_e8p_gemv_planes_rows": "planes:16 qidxs:16 grid:64 y:1 rows=2 n=256 k=4096 stream",
    "quip_gemv_planes_rows_mode": "planes:16 qidxs:16 grid:64 grid2:?1 y:1 rows=2 n=256 k=4096 mode=0 stream",
    "quip_e8p_gemv_fused": "in:f qidxs:g16 grid:64 ys:g1 ns:n count=2 k=4096 stream",
    "quip_e8p_gemv_kernel_choice": "ns:n count=2 k=4096",
    "quip_e8p_x_to_planes": "x:16 planes:16 k=4096 stream",
    "quip_e8p_mm_origorder": _MM.format(t=_T1.format(a=1)),
    "quip_e8p_mm_origorder_ws": _MM.format(t=_T1.format(a=1))[:-len(" stream")] + " workspace:?1 ws_bytes=1048576 stream",
    "quip_e8prvq3_mm_origorder": _MM.format(t="grid:1 grid2:1 scale=0.5 "),
    "quip_e8prvq4_mm_origorder": _MM.format(t=_T.format(a=1)),
    "quip_d4_mm_origorder": _MM.format(t=_T1.format(a=1)),
    "quip_hi_mm_origorder": _MM.format(t=""),
    "quip_e8p_mm_skinny": _SK.format(q=16, t=_T1.format(a=8)),
    "quip_e8prvq4_mm_skinny": _SK.format(q=16, t=_T.format(a=8)),
    "quip_e8prvq3_mm_skinny": _SK.format(q=4, t="grid:8 grid2:8 scale=0.5 "),
    "quip_d4_mm_skinny": _SK.format(q=16, t=_T1.format(a=8)),
    "quip_hi_mm_skinny": _SK.format(q=16, t=""),
    "quip_e8p_mm_batched": _BA.format(t=_T1.format(a=8)),
    "quip_e8prvq4_mm_batched": _BA.format(t=_T.format(a=8)),
    "quip_e8prvq3_mm_batched": _BA.format(t="grid:8 grid2:4 scale=0.5 "),
    "quip_d4_mm_batched": _BA.format(t=_T1.format(a=8)),
    "quip_hi_mm_batched": _BA.format(t=""),
    "quip_decompress_e8p_origorder": _DEC.format(t=_T1.format(a=1)),
    "quip_decompress_e8prvq3_origorder": _DEC.format(t="grid:1 grid2:1 scale=0.5 "),
    "quip_decompress_e8prvq4_origorder": _DEC.format(t=_T.format(a=1)),
    "quip_decompress_d4_origorder": _DEC.format(t=_T1.format(a=1)),
    "quip_decompress_hi_origorder": _DEC.format(t=""),
}
NOT_AT_ZERO = ("scale", "ws_bytes", "mode")     # numbers whose 0 is a valid value (their rows are written out below)
NS = (256, 512, 256, 256)                       # the group's problems; the host arrays hold four elements whatever count is
# a shape only the K-splitting kernel takes (rows longer than 28672 as the kernels see them).  These are the only rows whose
# answer passes through device_cu_count(): the K-splitting kernel's planner reads it before it finds that the split of K
# needs a workspace.  They are not device independent by construction, only by the choice of few rows: with n = 16 a
# workgroup holds one accumulator unit however many row blocks the CU count makes, so whether K is split follows from k
# alone.  (A machine without a GPU and an MI355X both resolve to 256 CUs.)
LONG = {"n": 16, "ns[0]": 16, "ns[1]": 16, "k": 57344}
FUSED_PTRS = ("x", "z", "post_scale", "residual", "h_out", "rms_weight")


def parse(entry):
    """[(name, kind, value)]: kind 'ptr' (value: (alignment, optional)), 'g' (value: the elements' alignment), 'n', 'f',
    'num' (value: the default), 'stream'"""
    out = []
    for tok in SPECS[entry].split():
        if tok == "stream":
            out.append((tok, "stream", None))
        elif "=" in tok:
            name, v = tok.split("=")
            out.append((name, "num", float(v) if name == "scale" else int(v)))
        else:
            name, a = tok.split(":")
            if a in ("n", "f"):
                out.append((name, a, None))
            elif a[0] == "g":
                out.append((name, "g", int(a[1:])))
            else:
                out.append((name, "ptr", (int(a.lstrip("?")), a.startswith("?"))))
    return out


_buf = (ctypes.c_char * 8192)()
P64 = ((ctypes.addressof(_buf) + 63) & ~63) + 1024
_HERE = object()


def _at(f, dflt=P64):
    return dflt if f is _HERE else None if f is None else P64 + f


def call(lib, entry, faults):
    """`entry` on valid arguments except at `faults`, {argument: value}: a pointer's value is None (NULL) or the number of
    bytes it is off by (0: an optional pointer that is there), "planes[1]" names an element of a pointer array, "ns[0]" a
    problem's n, "in.z" a member of quip_gemv_fused_in, "in.pre_scale[0]" an element of its array."""
    from quip_for_all_amd import capi
    keep, args = [], []
    for name, kind, value in parse(entry):
        f = faults.get(name, _HERE)
        if kind == "stream":
            args.append(None)
        elif kind == "num":
            args.append(value if f is _HERE else f)
        elif kind == "g":
            arr = (ctypes.c_void_p * 4)(*[_at(faults.get(f"{name}[{i}]", _HERE)) for i in range(4)])
            keep.append(arr)
            args.append(_at(f, ctypes.addressof(arr)))
        elif kind == "n":
            arr = (ctypes.c_int32 * 4)(*[faults.get(f"ns[{i}]", NS[i]) for i in range(4)])
            keep.append(arr)
            args.append(_at(f, ctypes.addressof(arr)))
        elif kind == "f":
            s = capi.GemvFusedIn()
            s.x = _at(faults.get("in.x", _HERE))
            for m in FUSED_PTRS[1:]:
                setattr(s, m, _at(faults.get("in." + m, _HERE), None))
            for i in range(3):
                s.pre_scale[i] = _at(faults.get(f"in.pre_scale[{i}]", _HERE))
                s.scale[i] = 1.0
            s.z_scale, s.rms_eps = 1.0, 1e-5
            keep.append(s)
            args.append(_at(f, ctypes.addressof(s)))
        else:
            args.append(_at(f))
    return getattr(lib, entry)(*args)


def row_id(entry, faults):
    return entry + " " + " ".join(f"{k}={faults[k]}" for k in sorted(faults))


def recorded():
    """{row id: code} of the golden file, which keeps the rows entry by entry"""
    return {entry + " " + faults: code for entry, rows in json.load(open(GOLDEN))["rows"].items() for faults, code in rows.items()}


def table():
    """[(entry, faults)]: every row a call that is answered before any launch"""
    rows = []
    for entry in SPECS:
        spec = parse(entry)
        names = {n for n, _, _ in spec}
        put = lambda f: rows.append((entry, dict(f)))  # noqa: E731
        group = "count" in names
        elems = [(f"{n}[{i}]", v) for n, k, v in spec if k == "g" for i in range(2)]
        if "in" in names:
            elems += [(f"in.pre_scale[{i}]", 16) for i in range(2)]
        must = [n for n, k, v in spec if k in ("g", "n", "f") or (k == "ptr" and not v[1])] + [e for e, _ in elems]
        offs = [(n, v[0]) for n, k, v in spec if k == "ptr"] + elems
        empty = [n for n in EMPTY if n in names]
        # every required pointer NULL in turn, the array elements too
        for n in must:
            put({n: None})
        # every pointer off by 2, 4 and 8 (a table: 16 and 32 too) in turn: alone where that alone is refused, and beside
        # k = -1 always -- MISALIGNED where the entry looks at the pointer before it looks at k, else what it says to k
        for n, align in offs:
            for d in (2, 4, 8) + ((16, 32) if n.startswith("grid") else ()):
                if d % align:
                    put({n: d})
                put({n: d, "k": -1})
        # every count at 0 and at -1
        for n, k, _ in spec:
            if k == "num" and n not in NOT_AT_ZERO:
                put({n: 0})
                put({n: -1})
        if group:
            put({"count": 4})
            put({"ns[0]": 0})
            put({"ns[1]": -1})
        # the divisibility rules
        put({"k": 12})
        rvq3 = "rvq3" in entry
        if rvq3:
            put({"k": 4104})                                # k % 32 (and, skinny, k % 128)
        if "_skinny" in entry:
            put({"k": 4160})
            put({"n": 255})
            put({"m": 32 * 65535 + 1})
        if "_batched" in entry:
            put({"k": 4128})
            put({"n": 255})
            put({"m": 1 << 31})
        if "rows" in names and "planes" in names:
            put({"rows": 6})                                # more rows than one pass takes
            put({"k": LONG["k"]})
        if "mode" in names:
            put({"mode": 7})
            put({"mode": -1})
            put({"mode": 40, "k": 4128})                    # k % 64
            put({"mode": 40, "grid2": None})
            put({"mode": 7, "planes": 2})
            put({"mode": 40, "k": 4128, "planes": 2})
        if entry == "quip_e8p_gemv_kernel_choice":
            put({"k": 28680})                               # neither kernel takes it
        if entry == "quip_e8p_gemv_fused":
            put({"in.x": None})
            put({"in.z": 0})                                # z without post_scale and h_out
            put({"in.z": 0, "in.post_scale": 0})
            put({"in.z": 0, "in.post_scale": 0, "in.h_out": 0, "in.residual": 0})      # h_out == residual
            put({"in.z": 2, "in.post_scale": 0, "in.h_out": 16})
            put({"in.z": 0, "in.post_scale": 2, "in.h_out": 16})
            put({"in.z": 0, "in.post_scale": 0, "in.h_out": 18})
            for m in ("x", "residual", "rms_weight"):
                for d in (2, 4, 8):
                    put({"in." + m: d})
                put({"in." + m: 2, "k": 12})
            put({"in.x": 2, "qidxs[0]": None})
            put({"in.x": None, "count": 0})
            put({"k": 4096 + 1024})                         # no power of two
            put({"k": 16384})
        # the K-splitting kernel's shape: without a workspace, and with one that is missing, short or misaligned
        if "planes" in names and "qidxs" in names and "rows" not in names:
            long = {k: v for k, v in LONG.items() if (k in names) or (group and k.startswith("ns["))}
            if "workspace" in names:
                put({**long, "workspace": None})
                put({**long, "ws_bytes": 0})
                put({**long, "ws_bytes": 64})
                put({**long, "workspace": 8})
                put({"workspace": 8, "k": 12})
                put({"workspace": 8, offs[0][0]: None})
            else:
                put(long)
        # two faults of different classes: which answer wins
        first, last = must[0], must[-1]
        if offs:
            other = next((n for n, a in offs if a > 2 and n != first), None) or next(n for n, _ in offs if n != first)
            put({first: None, other: 2})                                                  # NULL + misaligned, either order
            put({offs[0][0]: 2, last: None})
            put({other: 2, "k": 12})                                                      # misaligned + bad shape
        put({first: None, "k": 12})
        put({first: None, "k": -1})
        for bad in [n for n in ("m", "rows", "n", "count") if n in names][:1]:
            put({bad: -1, "k": 12})                                                       # bad shape + unsupported
        for i, e in enumerate(empty):
            # an empty dimension beside another fault: every pointer at the primary dimension, the first at the others
            for n, align in (offs if i == 0 else offs[:1]):
                put({e: 0, n: 2})
                if n.startswith("grid") and align > 2:
                    put({e: 0, n: 4})
            for n in (must if i == 0 else must[:1]):
                put({e: 0, n: None})
            put({e: 0, "k": 12})
            put({e: 0, "k": -1})
            if "workspace" in names:
                put({e: 0, "workspace": 8})
        if len(empty) == 2:
            put({empty[0]: 0, empty[1]: -1})
            put({empty[0]: -1, empty[1]: 0})
    return rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    assert "QUIP_GEMV_V2" not in os.environ and "QUIP_GEMV_NIB" not in os.environ
    return capi.lib()


def test_the_table_covers_every_product_entry_and_names_each_row_once():
    import re
    from quip_for_all_amd import capi
    pat = re.compile(r"quip_(e8p|d4|e8prvq3)_gemv_planes(_ws|_group|_group_ws|_v2|_rows)?$|quip_gemv_planes_rows_mode$"
                     r"|quip_e8p_gemv_(fused|kernel_choice)$|quip_e8p_x_to_planes$|quip_e8p_mm_origorder_ws$"
                     r"|quip_\w+_mm_(origorder|skinny|batched)$|quip_decompress_\w+_origorder$")
    want = {n for n in capi.SIGNATURES if pat.match(n)}
    assert set(SPECS) == want and len(want) == 36
    for entry in SPECS:
        assert len(parse(entry)) == len(capi.SIGNATURES[entry]), entry
    ids = [row_id(*r) for r in table()]
    assert len(ids) == len(set(ids))


def test_every_answer_is_the_recorded_one(lib):
    golden = recorded()
    rows = table()
    assert sorted(row_id(*r) for r in rows) == sorted(golden)              # the table is the recorded one, nothing dropped
    got = {row_id(entry, faults): call(lib, entry, faults) for entry, faults in rows}
    wrong = {k: (ANSWERS.get(golden[k], golden[k]), ANSWERS.get(v, v)) for k, v in got.items() if v != golden[k]}
    assert not wrong, f"{len(wrong)} of {len(got)} rows answer another code (recorded, now): {wrong}"
    assert set(golden.values()) == set(ANSWERS)                            # the four refusal codes and QUIP_OK all occur
    for entry, faults in rows:                                             # QUIP_OK: only where a dimension is empty
        assert golden[row_id(entry, faults)] != 0 or any(faults.get(e) == 0 for e in EMPTY), row_id(entry, faults)
