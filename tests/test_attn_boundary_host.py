"""What the attention entry points of the C ABI refuse, and with which code, without a GPU: the fourteen quip_rope_attn_*
calls and quip_qk_norm_rows_f16 against tests/golden/attn_refusals.json, recorded by tools/attn_refusals_golden.py from the
library of the commit before the attention host path was unified.  Every row is refused before any launch (NULL stream,
host scratch for every pointer), so the comparison is code for code: which pointers an entry looks at, which alignment it
asks of each, and which code wins where two things are wrong at once (NULL, then MISALIGNED, then window, then the
launcher's BAD_SHAPE, then UNSUPPORTED)."""
import ctypes
import json
import os

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "attn_refusals.json")
REFUSALS = {-1: "NULL_POINTER", -2: "BAD_SHAPE", -3: "MISALIGNED", -5: "UNSUPPORTED"}

# An entry's arguments in the order of include/quip_mi355.h.  name:A -- a pointer the entry wants A-byte aligned (1: it
# does not look); name:?16 -- the optional workspace (NULL is a legal value, so it has no NULL row); name:z -- a host
# array of three 16-byte-aligned device pointers (elements name[i]); name:h -- a host int32 array (the segment lists);
# name=V -- a number with a valid value; stream -- always NULL.
_QKV, _CSP = "q:16 k:16 v:16", "cos:1 sin:1 pos:{pos}"
_DEC = _QKV + " " + _CSP + " kcache:16 vcache:16 out:1"
_ROWS = _QKV + " cos:16 sin:16 pos:8 {cache} out:16"
_PAGED = _QKV + " " + _CSP.format(pos=8) + " table:4 kpool:16 vpool:16 out:1"
_SHAPE = "heads=4 kv_heads=2 head_dim=64 max_len=128"
_SEGS = "seg_slot:h seg_rows:h nseg=3"
_ZSHAPE = "heads=32 kv_heads=32 head_dim=128 max_len=128"
_Z = "z:z post:z scales:1 cos:1 sin:1 pos:1 kcache:16 vcache:16 out:1 " + _ZSHAPE
SPECS = {
    "quip_rope_attn_decode_f16": _DEC.format(pos=1) + " " + _SHAPE + " scale=0.125 workspace:?16 stream",
    "quip_rope_attn_decode_window_f16": _DEC.format(pos=1) + " " + _SHAPE + " scale=0.125 window=0 workspace:?16 stream",
    "quip_rope_attn_decode_batched_f16": _DEC.format(pos=8) + " batch=5 " + _SHAPE + " scale=0.125 window=0 workspace:?16 stream",
    "quip_rope_attn_decode_batched_start_f16": _DEC.format(pos=8) + " batch=5 " + _SHAPE
                                               + " scale=0.125 window=0 workspace:?16 stream start:8",
    "quip_rope_attn_chunk_f16": _ROWS.format(cache="kcache:16 vcache:16") + " rows=76 " + _SHAPE + " scale=0.125 window=0 stream",
    "quip_rope_attn_ragged_f16": _ROWS.format(cache="kcache:16 vcache:16") + " rows=76 " + _SHAPE + " batch=5 " + _SEGS
                                 + " scale=0.125 window=0 stream",
    "quip_rope_attn_decode_paged_f16": _PAGED + " batch=5 " + _SHAPE + " n_pages=8 max_pages=2 scale=0.125 window=0 workspace:?16 stream",
    "quip_rope_attn_ragged_paged_f16": _ROWS.format(cache="table:4 kpool:16 vpool:16") + " rows=76 " + _SHAPE
                                       + " batch=5 n_pages=8 max_pages=2 " + _SEGS + " scale=0.125 window=0 stream",
    "quip_rope_attn_decode_paged_f8": _PAGED + " batch=5 " + _SHAPE
                                      + " n_pages=8 max_pages=2 scale=0.125 window=0 workspace:?16 stream k_exp=0 v_exp=0",
    "quip_rope_attn_ragged_paged_f8": _ROWS.format(cache="table:4 kpool:16 vpool:16") + " rows=76 " + _SHAPE
                                      + " batch=5 n_pages=8 max_pages=2 " + _SEGS + " scale=0.125 window=0 stream k_exp=0 v_exp=0",
    "quip_rope_attn_decode_qknorm_f16": _DEC.format(pos=1) + " " + _SHAPE
                                        + " scale=0.125 window=0 workspace:?16 stream q_weight:16 k_weight:16 eps=1e-6",
    "quip_rope_attn_decode_batched_qknorm_f16": _DEC.format(pos=8) + " batch=5 " + _SHAPE
                                                + " scale=0.125 window=0 workspace:?16 stream q_weight:16 k_weight:16 eps=1e-6",
    "quip_rope_attn_decode_z_f16": _Z + " scale=0.088 workspace:?16 stream",
    "quip_rope_attn_decode_z_window_f16": _Z + " scale=0.088 window=0 workspace:?16 stream",
    "quip_qk_norm_rows_f16": "q:16 k:16 q_weight:16 k_weight:16 rows=7 heads=4 kv_heads=2 head_dim=64 eps=1e-6 stream",
}
SEG_VALUES = {"seg_slot": (2, 0, 3), "seg_rows": (5, 1, 70)}       # the valid lists: 76 rows into slots of batch = 5
NOT_AT_ZERO = ("scale", "eps", "window", "k_exp", "v_exp")        # numbers whose 0 (and, for the exponents, -1) is a valid value


def parse(entry):
    """[(name, kind, value)]: kind 'ptr' (value: (alignment, optional)), 'z', 'h', 'num' (value: the default), 'stream'"""
    out = []
    for tok in SPECS[entry].split():
        if tok == "stream":
            out.append((tok, "stream", None))
        elif "=" in tok:
            name, v = tok.split("=")
            out.append((name, "num", float(v) if name in ("scale", "eps") else int(v)))
        else:
            name, a = tok.split(":")
            out.append((name, a, None) if a in ("z", "h") else (name, "ptr", (int(a.lstrip("?")), a.startswith("?"))))
    return out


_buf = (ctypes.c_char * 4096)()
P16 = ((ctypes.addressof(_buf) + 15) & ~15) + 256
_HERE = object()


def call(lib, entry, faults):
    """`entry` on valid arguments except at `faults`, {argument: value}: a pointer's value is None (NULL) or the number of
    bytes it is off by, "z[1]" names an element of a pointer array, "seg_slot_values" / "seg_rows_values" replace a segment
    list (nseg and rows follow the lists unless they are faults themselves)."""
    keep, args = [], []
    seg = {n: tuple(faults.get(n + "_values", v)) for n, v in SEG_VALUES.items()}

    def at(base, f):
        return base if f is _HERE else None if f is None else base + f
    for name, kind, value in parse(entry):
        f = faults.get(name, _HERE)
        if kind == "stream":
            args.append(None)
        elif kind == "num":
            if f is _HERE and ("seg_slot_values" in faults or "seg_rows_values" in faults):
                value = {"nseg": len(seg["seg_slot"]), "rows": sum(seg["seg_rows"])}.get(name, value)
            args.append(value if f is _HERE else f)
        elif kind == "z":
            arr = (ctypes.c_void_p * 3)(*[at(P16, faults.get(f"{name}[{i}]", _HERE)) for i in range(3)])
            keep.append(arr)
            args.append(at(ctypes.addressof(arr), f))
        elif kind == "h":
            arr = (ctypes.c_int32 * (len(seg[name]) + 4))(*seg[name])      # (room behind the list for a pointer that is off)
            keep.append(arr)
            args.append(at(ctypes.addressof(arr), f))
        else:
            args.append(at(P16, f))
    return getattr(lib, entry)(*args)


def row_id(entry, faults):
    return entry + " " + " ".join(f"{k}={faults[k]}" for k in sorted(faults))


def table():
    """[(entry, faults)]: every row a call that is refused before any launch"""
    rows = []
    for entry in SPECS:
        spec = parse(entry)
        names = {n for n, _, _ in spec}
        put = lambda f: rows.append((entry, dict(f)))  # noqa: E731
        elems = [f"{n}[{i}]" for n, k, _ in spec if k == "z" for i in range(3)]
        must = [n for n, k, v in spec if k in ("z", "h") or (k == "ptr" and not v[1])]           # NULL is refused
        offs = [(n, v[0]) for n, k, v in spec if k == "ptr"] + [(n, 1) for n, k, _ in spec if k == "h"] + [(e, 16) for e in elems]
        # every pointer NULL in turn
        for n in must + elems:
            put({n: None})
        # every pointer off by 2, 4 and 8 in turn: alone where that alone is refused, and beside heads = 0 always -- MISALIGNED
        # where the entry looks at the pointer, the launcher's BAD_SHAPE where it does not, so a pointer that joins or leaves
        # an entry's set shows either way.  (The z / post arrays themselves are host arrays the entry reads: not moved.)
        for n, align in offs:
            for d in (2, 4, 8):
                if d % align:
                    put({n: d})
                put({n: d, "heads": 0})
        # numbers
        for n, k, _ in spec:
            if k == "num" and n not in NOT_AT_ZERO:
                put({n: 0})
                put({n: -1})
        if entry != "quip_qk_norm_rows_f16":                # (q and k are normalised head by head: no rule between the counts)
            put({"heads": 6, "kv_heads": 4})
        put({"head_dim": 96})
        put({"head_dim": 256})
        if "window" in names:
            put({"window": -1})
        batched = "batch" in names and "rows" not in names
        if batched:
            put({"batch": 65536})
        if "max_pages" in names:
            put({"max_len": 2 * 64 + 1})
            if batched:                                     # (the decode launch keeps the table row in LDS; the ragged one does not)
                put({"max_pages": 8193, "max_len": 128})
                put({"max_pages": 8193, "max_len": 8193 * 64 + 1})                    # bad shape + unsupported
        if "k_exp" in names:
            for e in (8, -9):
                put({"k_exp": e})
                put({"v_exp": e})
            put({"k_exp": 8, "head_dim": 96})                                         # bad shape + unsupported
        if entry == "quip_qk_norm_rows_f16":
            put({"heads": 65537})
            put({"kv_heads": 65537})
            put({"rows": 1 << 40, "heads": 65536, "kv_heads": 65536})              # more workgroups than a grid holds
        # the segment lists (tests/test_ragged_attn_host.py)
        if "nseg" in names:
            put({"seg_slot_values": tuple(range(33)), "seg_rows_values": (1,) * 33, "batch": 40})
            put({"seg_rows_values": (5, 0, 70)})
            put({"seg_rows_values": (5, -1, 70), "rows": 74})
            put({"rows": 75})
            put({"rows": 77})
            put({"seg_slot_values": (2, 5, 3)})
            put({"seg_slot_values": (2, -1, 3)})
            put({"seg_slot_values": (2, 0, 2)})
            put({"seg_rows_values": (64 * 65535 + 1,), "seg_slot_values": (1,)})      # more query tiles than a grid holds
            put({"seg_slot_values": (2, 0, 2), "head_dim": 96})                      # bad shape + unsupported
            put({"rows": 75, "seg_rows_values": (64 * 65535 + 1,), "seg_slot_values": (1,)})
            put({"seg_rows_values": (64 * 65535 + 1,), "seg_slot_values": (1,), "head_dim": 96})
        # two faults of different classes: which code wins
        first, last = must[0], must[-1]
        other = next(n for n, a in offs if a > 2 and n != first)
        put({first: None, other: 2})                                                  # NULL + misaligned, either order
        put({offs[0][0]: 2, last: None})
        put({first: None, "head_dim": 96})
        put({first: None, "heads": 0})
        put({other: 2, "head_dim": 96})                                               # misaligned + unsupported
        put({"heads": 6, "kv_heads": 4, "head_dim": 96})                              # bad shape + unsupported
        put({"heads": 0, "head_dim": 256})
        if "window" in names:
            put({"window": -1, first: None})
            put({"window": -1, other: 2})
            put({"window": -1, "head_dim": 96})
            put({"window": -1, "heads": 0})
        if "workspace" in names:
            put({"workspace": 8, "head_dim": 96})
            if "window" in names:
                put({"workspace": 8, "window": -1})
        if elems:
            put({"z[0]": 2, "z[1]": None})               # the element checks go element by element: the first fault wins
            put({"z[0]": None, "z[1]": 2})
            put({"post[0]": 2, "z[1]": None})
            put({"z[2]": None, "kcache": 2})
            put({"post[2]": 8, "kcache": None})
    return rows


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    from quip_for_all_amd import capi
    return capi.lib()


def test_the_table_covers_every_attention_entry_and_names_each_row_once():
    from quip_for_all_amd import capi
    want = {n for n in capi.SIGNATURES if n.startswith("quip_rope_attn_") and n.endswith(("_f16", "_f8"))} | {"quip_qk_norm_rows_f16"}
    assert set(SPECS) == want and len(want) == 15
    for entry in SPECS:
        assert len(parse(entry)) == len(capi.SIGNATURES[entry]), entry
    ids = [row_id(*r) for r in table()]
    assert len(ids) == len(set(ids))


def test_every_refusal_is_the_recorded_one(lib):
    golden = json.load(open(GOLDEN))["rows"]
    rows = table()
    assert sorted(row_id(*r) for r in rows) == sorted(golden)              # the table is the recorded one, nothing dropped
    got = {row_id(entry, faults): call(lib, entry, faults) for entry, faults in rows}
    wrong = {k: (REFUSALS.get(golden[k], golden[k]), REFUSALS.get(v, v)) for k, v in got.items() if v != golden[k]}
    assert not wrong, f"{len(wrong)} of {len(got)} rows answer another code (recorded, now): {wrong}"
    assert set(golden.values()) == set(REFUSALS)                           # all four refusal codes occur
