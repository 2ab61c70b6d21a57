"""Every plan kind of the Hadamard transform launches (had_plan(), csrc/hadamard.hip) once on the GPU, and the four
loose-argument C entry points.

Per kernel instantiation the smallest case of tests/golden/had_plans.json that reaches it and that the ops can express:
the plan hook says the case takes that instantiation, and the result equals, bit for bit, the route the project already
holds identical -- a batch against its single rows, a group against single calls, a single row against the same row inside
a batch of nine, a chain against transform-then-planes.  (had_tall_batch_kernel against single rows: the rule of
tests/test_gpu_ops.py, one fp16 ulp, its K-mix runs in another order.)  Three kinds have no such route -- the K-mix of a
long row sums k in one chain in a batch and in up to four thread groups for a single row, so the two differ in the last
bit, and the planes of a single long row have no second launch at all: ORACLE compares them with the float64 oracle
under the tolerance of tests/test_gpu_ops.py::test_matmul_hadU_cuda.  The existing GPU tests reach most kinds as well
(profiles/had_host_refactor.txt lists which); going through all of them here takes about a second and leaves no kind to
an argument about shapes.

The loose-argument entries are no longer what the ops call: one ctypes case each at n = 1024, K = 1 and n = 1408, K = 11,
bit identical to the op's result."""
import ctypes
import json

import numpy as np
import pytest
import torch

import quip_for_all_amd  # noqa: F401
from quip_for_all_amd import capi
from tests import test_had_plan_host as T
from tests.test_gpu_ops import _same_or_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OPS = torch.ops.quip_lib
LETTERS = {"p": "pre", "2": "pre2", "g": "gate", "r": "rms_weight", "o": "post", "b": "bias", "s": "residual"}


def _expressible(case):
    planes, K, ns, rows, chain, vectors, off, din, dout = case
    count, every = len(ns), lambda c: all(c in v for v in vectors) or not any(c in v for v in vectors)  # noqa: E731
    if off or din or dout:
        return False
    if chain:
        return bool(planes) and all("p" in v and set(v) <= set("pr") for v in vectors) and every("r")     # (the op's pre: Tensor[])
    if count == 1:
        return set(vectors[0]) <= (set("prg") if planes else set(LETTERS))
    if planes:
        return rows == 1 and all(set(v) <= set("prg") for v in vectors) and every("r") and every("g")
    return all(set(v) <= set("p2obsr") for v in vectors) and every("r")


def _cases():
    """{kind: its smallest expressible case of the golden table}"""
    with open(T.GOLDEN) as f:
        golden = json.load(f)
    best = {}
    for case, plan in zip(T.cases(), T.decode(golden)):
        if plan[0] != 0 or plan[1] is None or not _expressible(case):
            continue
        kind, size = plan[1], (sum(map(len, case[5])), sum(case[2]), case[1], case[3], len(case[2]), case[4])
        if kind not in best or size < best[kind][0]:
            best[kind] = (size, case)
    return {k: c for k, (_, c) in sorted(best.items())}


CASES = _cases()


ORACLE = {"had_fast_kernel<false, false, 256, false, 0>", "had_fast_kernel<true, false, 256, false, 0>",
          "had_fast_kernel<true, false, 1024, false, 0>"}


def _against_the_oracle(p, planes):
    """a transform without element-wise vectors against oracle.matmul_hadU, the tolerance of test_matmul_hadU_cuda; planes
    hold X = rint(v * 2^sh): half a unit of 2^-sh on top"""
    from oracle import quip_oracle as O
    from tests.test_gpu_ops import _decode_planes
    assert all(t is None for t in p.v.values())
    ref = O.matmul_hadU(p.x.cpu().numpy().astype(np.float64), None if p.had is None else p.had.cpu().numpy().astype(np.float64),
                        p.K, p.n, transpose=bool(planes)) * np.sqrt(p.n // p.K) * p.scale
    tol = 2.0 ** -10 * np.abs(ref) + 2.0 ** -18 * np.linalg.norm(ref, axis=1, keepdims=True) + 1e-6
    if planes:
        images = p.planes_rows() if p.rows > 1 else p.planes(0)[None]
        got = np.empty_like(ref)
        for r in range(p.rows):
            X, sh, _ = _decode_planes(images[r], p.n)
            got[r] = X[:p.n] * 2.0 ** -sh
            tol[r] += 0.5 * 2.0 ** -sh
    else:
        got = p.f16().cpu().numpy().astype(np.float64)
    assert np.all(np.abs(got - ref) <= tol), float((np.abs(got - ref) / tol).max())


def test_every_plan_kind_has_a_case():
    assert set(CASES) == set(capi.had_plan_kinds())


def _rand(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen, device=DEV) * scale).half()


def _used(planes, n):
    """the bytes of a plane image that carry a result: the digits and the shift word"""
    return planes[..., :3 * ((n + 511) // 512 * 512) + 4]


class _Problem:
    """one problem's operands on the device"""

    def __init__(self, gen, n, K, rows, letters, had=None):
        self.n, self.K, self.rows = n, K, rows
        self.x = _rand(gen, rows, n)
        self.had = had if had is not None else None if K == 1 else _rand(gen, K, K, scale=K ** -0.5)
        self.scale = float(0.9 / np.sqrt(n // K))
        v = {name: None for name in LETTERS.values()}
        for c in letters:
            name = LETTERS[c]
            v[name] = _rand(gen, rows, n) if name in ("gate", "residual") else 1 + _rand(gen, n, scale=0.25) if name != "bias" else _rand(gen, n)
        self.v = v

    def f16(self, r=None):
        """the single call on fp16 rows: all of them, or row r alone"""
        s, v = slice(None) if r is None else slice(r, r + 1), self.v
        cut = lambda t: None if t is None else t[s]  # noqa: E731
        return OPS.had_transform_fused(self.x[s], self.n, self.n, self.K, self.had, False, v["pre"], v["pre2"], v["post"], v["bias"],
                                       self.scale, cut(v["residual"]), v["rms_weight"], 1e-5, cut(v["gate"]))

    def planes(self, r):
        v = self.v
        return OPS.had_transform_planes_fused(self.x[r:r + 1], self.n, self.K, self.had, True, v["pre"], self.scale, v["rms_weight"],
                                              1e-5, None if v["gate"] is None else v["gate"][r:r + 1])

    def planes_rows(self, x=None, gate=None):
        v = self.v
        return OPS.had_transform_planes_rows(self.x if x is None else x, self.n, self.K, self.had, True, v["pre"], self.scale,
                                             v["rms_weight"], 1e-5, v["gate"] if x is None else gate)


def _in_a_batch(gen, t, rows=9):
    return None if t is None else torch.cat([t, _rand(gen, rows - 1, t.shape[1])])


@pytest.mark.parametrize("kind", sorted(CASES))
def test_plan_kind_equals_the_route_held_identical(kind):
    case = CASES[kind]
    planes, K, ns, rows, chain, vectors = case[:6]
    assert T.plan(case)[:2] == [0, kind]
    gen = torch.Generator(device=DEV).manual_seed(len(kind) + sum(ns) + rows)
    same = _same_or_close if kind.startswith("had_tall_batch_kernel") else (lambda a, b, what: torch.equal(a, b) or pytest.fail(str(what)))
    count, n = len(ns), ns[0]
    if kind in ORACLE:
        assert count == 1 and not chain
        return _against_the_oracle(_Problem(gen, n, K, rows, vectors[0]), planes)
    if chain:
        L = n // K
        z, z_post, z_res = _rand(gen, 1, n), 1 + _rand(gen, n, scale=0.25), _rand(gen, 1, n) if chain == 1 else None
        z_had = None if K == 1 else _rand(gen, K, K, scale=K ** -0.5)
        ps = [_Problem(gen, n, K, 1, v) for v in vectors]
        rms = ps[0].v["rms_weight"]
        out = OPS.had_chain_planes_group(z, z_post, z_res, float(0.9 / np.sqrt(L)), n, [p.v["pre"] for p in ps], [p.scale for p in ps],
                                         rms, 1e-5, 0.0, K, z_had, [p.had for p in ps])
        h = OPS.had_transform_fused(z, n, n, K, z_had, False, None, None, z_post, None, float(0.9 / np.sqrt(L)), z_res, None, 1e-5, None)
        assert torch.equal(out[0], h)
        for p, got in zip(ps, out[1:]):
            p.x, p.v["rms_weight"] = h, rms
            assert torch.equal(_used(got, n), _used(p.planes(0), n))
        return
    if planes:
        if count == 1:
            p = _Problem(gen, n, K, rows, vectors[0])
            if rows == 1:      # the row alone against the same row at the head of a batch of nine
                got = p.planes(0)
                ref = p.planes_rows(_in_a_batch(gen, p.x), _in_a_batch(gen, p.v["gate"]))[0]
                assert torch.equal(_used(got, n), _used(ref, n))
            else:
                got = p.planes_rows()
                for r in (0, rows // 2, rows - 1):
                    assert torch.equal(_used(got[r], n), _used(p.planes(r), n)), r
            return
        shared = _Problem(gen, n, K, 1, vectors[0])
        ps = [shared] + [_Problem(gen, n, K, 1, v) for v in vectors[1:]]
        for p in ps[1:]:
            p.x, p.v["rms_weight"], p.v["gate"] = shared.x, shared.v["rms_weight"], shared.v["gate"]
        got = OPS.had_transform_planes_group(shared.x, n, K, [p.had for p in ps], True, [p.v["pre"] for p in ps],
                                             [p.scale for p in ps], shared.v["rms_weight"], 1e-5, shared.v["gate"])
        for p, g in zip(ps, got):
            assert torch.equal(_used(g, n), _used(p.planes(0), n))
        return
    ps = [_Problem(gen, ni, K, rows, v) for ni, v in zip(ns, vectors)]
    if count == 1:
        p = ps[0]
        got = p.f16()
        if rows == 1:
            q = _Problem(gen, n, K, 9, "", had=p.had)
            q.x, q.v = _in_a_batch(gen, p.x), {k: _in_a_batch(gen, t) if k in ("gate", "residual") else t for k, t in p.v.items()}
            same(got, q.f16()[:1], "row 0 of nine")
        else:
            for r in (0, rows // 2, rows - 1):
                same(got[r:r + 1], p.f16(r), r)
        return
    for p in ps[1:]:
        p.v["rms_weight"] = ps[0].v["rms_weight"]
    col = lambda name: [p.v[name] for p in ps]  # noqa: E731
    got = OPS.had_transform_group([p.x for p in ps], list(ns), n, K, [p.had for p in ps], False, col("pre2"), col("post"), col("bias"),
                                  [p.scale for p in ps], col("residual"), col("pre"), ps[0].v["rms_weight"], 1e-5,
                                  list(ns) if len(set(ns)) > 1 else None)
    for i, (p, g) in enumerate(zip(ps, got)):
        for r in sorted({0, rows - 1}):
            same(g[r:r + 1], p.f16(r), (i, r))


# ---- the loose-argument entry points, which the ops no longer call -------------------------------------------------------
@pytest.mark.parametrize("n,K", [(1024, 1), (1408, 11)])
@pytest.mark.parametrize("entry", ["quip_had_transform_f16", "quip_had_transform_fused_f16", "quip_had_transform_planes",
                                   "quip_had_transform_planes_fused"])
def test_loose_argument_entry_equals_the_op(entry, n, K):
    gen = torch.Generator(device=DEV).manual_seed(n + K)
    fused, planes = "fused" in entry, "planes" in entry
    rows = 1 if planes else 3
    p = _Problem(gen, n, K, rows, ("prg" if planes else "p2obsrg") if fused else ("p" if planes else "p2ob"))
    v, L = p.v, capi.lib()
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    fusion = capi.HadFusion(ptr(v["residual"]), ptr(v["rms_weight"]), ptr(v["gate"]), 1e-5)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    with torch.cuda.device(DEV):
        if planes:
            want = p.planes(0)
            got = torch.empty_like(want)
            args = (p.x.data_ptr(), got.data_ptr(), n, n, K, ptr(p.had), 1, ptr(v["pre"]), p.scale)
        else:
            want = p.f16()
            got = torch.empty_like(want)
            args = (p.x.data_ptr(), got.data_ptr(), rows, n, n, n, K, ptr(p.had), 0, ptr(v["pre"]), ptr(v["pre2"]), ptr(v["post"]),
                    ptr(v["bias"]), p.scale)
        capi.check(getattr(L, entry)(*args, *((ctypes.byref(fusion),) if fused else ()), stream), entry)
        torch.cuda.synchronize()
    assert torch.equal(_used(got, n), _used(want, n)) if planes else torch.equal(got, want)
