"""The operand checks of the eight transform ops (register_lib._check_had and what stands around it), without a GPU: each
_had_*_cuda function called directly on CPU tensors that are wrong in one respect answers ValueError("quip_lib: ...")
before the library is touched.  Every row but those of NEW was refused the same way before the ops got one check; the
rows of NEW reached the kernel unchecked then (profiles/had_host_refactor.txt)."""
import pytest
import torch

import quip_for_all_amd  # noqa: F401
from quip_for_all_amd import capi, register_lib as R

N, K, KK = 1024, 1, 11                    # K == 1 rows; the K > 1 rows take n = 11 * 128
F16 = torch.float16


def h(*shape, dtype=F16):
    return torch.zeros(*shape, dtype=dtype)


def valid(op, K=1):
    """positional arguments of register_lib._<op>_cuda, all valid, as a dict in the op's order"""
    n = N if K == 1 else K * 128
    had = None if K == 1 else h(K, K)
    if op in ("had_transform", "had_transform_fused"):
        a = dict(x=h(2, n), out_features=n, n=n, K=K, had=had, transpose=False, pre=h(n), pre2=h(n), post=h(n), bias=h(n), scale=1.0)
        if op == "had_transform_fused":
            a.update(residual=h(2, n), rms_weight=h(n), rms_eps=1e-5, gate=h(2, n))
        return a
    if op == "had_transform_planes":
        return dict(x=h(1, n), n=n, K=K, had=had, transpose=True, pre=h(n), scale=1.0)
    if op in ("had_transform_planes_fused", "had_transform_planes_rows"):
        rows = 1 if op.endswith("fused") else 3
        return dict(x=h(rows, n), n=n, K=K, had=had, transpose=True, pre=h(n), scale=1.0, rms_weight=h(n), rms_eps=1e-5,
                    gate=h(rows, n), resid_scale=0.0)
    if op == "had_transform_planes_group":
        return dict(x=h(1, n), n=n, K=K, had=[had, had], transpose=True, pre=[h(n), h(n)], scale=[1.0, 1.0], rms_weight=h(n),
                    rms_eps=1e-5, gate=h(1, n), resid_scale=0.0)
    if op == "had_chain_planes_group":
        return dict(z=h(1, n), z_post=h(n), z_residual=h(1, n), z_scale=1.0, n=n, pre=[h(n), h(n)], scale=[1.0, 1.0],
                    rms_weight=h(n), rms_eps=1e-5, resid_scale=0.0, K=K, z_had=had, had=[had, had])
    assert op == "had_transform_group"
    return dict(x=[h(2, n), h(2, n)], out_features=[n, n], n=n, K=K, had=[had, had], transpose=False, pre2=[h(n), h(n)],
                post=[h(n), h(n)], bias=[None, None], scale=[1.0, 1.0], residual=[h(2, n), None], pre=[h(n), None],
                rms_weight=None, rms_eps=1e-5, ns=None)


OPS = ("had_transform", "had_transform_planes", "had_transform_fused", "had_transform_planes_fused",
       "had_transform_planes_group", "had_transform_planes_rows", "had_transform_group", "had_chain_planes_group")


def _bad(t, how):
    """a tensor (or, of a list, its first tensor) wrong in one respect"""
    if isinstance(t, list):
        return [_bad(t[0], how)] + t[1:]
    if how == "dtype":
        return t.float()
    if how == "strided":
        return torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype)[..., ::2]
    if how == "short":
        return t.reshape(-1)[:-1].clone()
    assert how == "shape"
    return torch.zeros(t.shape[0] + 1, t.shape[1], dtype=t.dtype)


def table():
    """[(op, fault name, arguments)]"""
    rows = []
    for op in OPS:
        a = valid(op)
        xk = "z" if "z" in a else "x"
        put = lambda name, **kw: rows.append((op, name, {**a, **kw}))  # noqa: E731
        put(xk + " float32", **{xk: _bad(a[xk], "dtype")})
        x0 = a[xk][0] if isinstance(a[xk], list) else a[xk]
        put(xk + " 1-D", **{xk: [x0[0]] + a[xk][1:] if isinstance(a[xk], list) else x0[0]})
        for v in ("had", "pre", "pre2", "post", "bias", "rms_weight", "z_post"):
            if a.get(v) is None or (isinstance(a[v], list) and a[v][0] is None):
                continue
            for how in ("dtype", "strided", "short"):
                put(f"{v} {how}", **{v: _bad(a[v], how)})
        for v in ("gate", "residual", "z_residual"):
            if a.get(v) is not None:
                put(f"{v} shape", **{v: _bad(a[v], "shape")})
                put(f"{v} dtype", **{v: _bad(a[v], "dtype")})
                put(f"{v} strided", **{v: _bad(a[v], "strided")})
        if op in ("had_transform_planes", "had_transform_planes_fused", "had_chain_planes_group"):
            put("two rows", **{xk: h(2, N)}, **({"gate": h(2, N)} if "gate" in a else {}))
        put("K > 1 without had", **{**valid(op, KK), "had": [None, None] if isinstance(a["had"], list) else None})
        put("had of another K", **{**valid(op, KK), "had": [h(3, 3), h(3, 3)] if isinstance(a["had"], list) else h(3, 3)})
        put("K does not divide n", K=3)
        put("n < in_features", n=N // 2)
        if "out_features" in a:
            put("out_features > n", out_features=[N + 1, N] if isinstance(a["out_features"], list) else N + 1)
        if isinstance(a["pre"], list):        # the grouped ops
            for v in [k for k, t in a.items() if isinstance(t, list) and k not in ("x", "pre")]:
                put(f"{v} one entry short", **{v: a[v][:-1]})
            put("count 0", **{k: [] for k, t in a.items() if isinstance(t, list)})
            put("count 4", **{k: t + t for k, t in a.items() if isinstance(t, list)})
        if op == "had_transform_planes_group":
            put("three rows for two problems", x=h(3, N), gate=None)
        if op == "had_chain_planes_group":
            put("K > 1 without z_had", **{**valid(op, KK), "z_had": None})
            put("z_had of another K", **{**valid(op, KK), "z_had": h(3, 3)})
            put("z_had float32", **{**valid(op, KK), "z_had": h(KK, KK, dtype=torch.float32)})
            put("K == 1 had float32", had=[h(1, 1, dtype=torch.float32), None])
        if op == "had_transform_group":
            put("rows differ", x=[h(2, N), h(3, N)])
            put("widths differ without ns", x=[h(2, N), h(2, N // 2)])
            put("ns with rms_weight", ns=[N, N], rms_weight=h(N))
            put("ns one entry short", ns=[N])
            put("ns with K > 1", **{**valid(op, KK), "ns": [KK * 128, KK * 128]})
    return rows


# refused only since the ops share one check: a consumer factor of one element beside K == 1, which was looked at for its
# length and then ignored; and, which no CPU tensor can show, a gate on another device than x in had_transform_planes_rows
NEW = {("had_chain_planes_group", "K == 1 had float32")}


def call(op, args):
    return getattr(R, f"_{op}_cuda")(*args.values())


def test_every_op_has_rows_and_each_is_named_once():
    rows = table()
    assert {op for op, _, _ in rows} == set(OPS) and len({(op, name) for op, name, _ in rows}) == len(rows)
    assert NEW <= {(op, name) for op, name, _ in rows}


@pytest.mark.parametrize("op", OPS)
def test_a_wrong_operand_is_refused_before_the_library(op, monkeypatch):
    def reached(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(capi, "lib", reached)
    for name, args in [(n, a) for o, n, a in table() if o == op]:
        with pytest.raises(ValueError, match="^quip_lib: "):
            call(op, args)
            pytest.fail(f"{op}: {name} was not refused")


def test_a_message_names_the_op_and_the_argument():
    a = valid("had_transform_planes_rows")
    with pytest.raises(ValueError, match="had_transform_planes_rows: gate must have x's shape"):
        call("had_transform_planes_rows", {**a, "gate": h(2, N)})
    a = valid("had_transform_group")
    with pytest.raises(ValueError, match="had_transform_group: post must be contiguous float16"):
        call("had_transform_group", {**a, "post": [h(N).float(), h(N)]})
    with pytest.raises(ValueError, match="had_transform: pre has 1023 elements, expected 1024"):
        call("had_transform", {**valid("had_transform"), "pre": h(N - 1)})


def test_problems_are_built_by_field_name_with_the_headers_defaults():
    t = h(8)
    pr = R._had_problem(x=t, in_features=8, out_features=8, **R._layout(R.HI_PLANES))
    assert pr.x == t.data_ptr() and pr.out is None and (pr.in_features, pr.out_features) == (8, 8)
    assert (pr.scale, pr.z_scale, pr.resid_scale, pr.planes_layout, pr.n) == (1.0, 1.0, 0.0, 2, 0)
    assert abs(pr.rms_eps - 1e-5) < 1e-12 and pr.z is None and pr.z_had is None
    assert R._layout(0.5) == {"resid_scale": 0.5, "planes_layout": 0}
    with pytest.raises(AssertionError):
        R._had_problem(pre=t)                      # the header's name is pre_scale


def test_planes_numel_is_the_librarys_planes_bytes():
    import __graft_entry__ as g
    g.build_library(verbose=False)
    L = capi.lib()
    for n in (16, 64, 256, 512, 1024, 1408, 3072, 3584, 4096, 5120, 8192, 11008, 14336, 16384, 28672):
        assert R._planes_numel(n) == L.quip_e8p_planes_bytes(n), n
        assert R._planes_numel(n, 0.5) == R._planes_numel(n, R.HI_PLANES) == L.quip_e8p_planes_bytes(2 * n), n
