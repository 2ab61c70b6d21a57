"""Shape inference of every quip_lib op: one call per op (and per codebook / table mode) on `device="meta"` tensors
reaches the registered fake, with no GPU and without the native library.  Output shapes and dtypes are pinned."""
import torch

import quip_for_all_amd  # noqa: F401  (registers torch.ops.quip_lib.*)
from quip_for_all_amd import register_lib

F16, U8, I8, I16, I32, I64, F32 = torch.float16, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64, torch.float32
N, K_IN, M = 16, 256, 3          # out features, in features, activation rows
NP = 1024                        # planes ops: n of the transform (3 * 1024 + 16 bytes; 2 n virtual: 3 * 2048 + 16)
PL, PL2 = 3 * 1024 + 16, 3 * 2048 + 16


def t(*shape, dtype=F16):
    return torch.empty(*shape, dtype=dtype, device="meta")


# per codebook: Qidxs (N, columns) and the table arguments the mm / skinny / batched / decompress ops take
CODEBOOKS = {
    "e8p": (t(N, K_IN // 8, dtype=I16), (t(256, dtype=I64),)),
    "e8prvq4": (t(N, K_IN // 8, dtype=I32), (t(256, dtype=I64), 0.25)),
    "e8prvq3": (t(N, 3 * K_IN // 32, dtype=I32), (t(256, dtype=I64), t(256, dtype=I32), 0.25)),
    "d4": (t(N, K_IN // 4, dtype=U8), (t(256, 4),)),
    "hi": (t(N, K_IN // 8, dtype=I32), ()),
}


def _calls():
    """(op name, label, args, kwargs, expected [(shape, dtype)] of the output(s), or None for no output)"""
    x = t(M, K_IN)
    for cb, (q, tabs) in CODEBOOKS.items():
        yield f"{cb}_mm_origorder", cb, (x, q) + tabs, {}, [((M, N), F16)]
        yield f"{cb}_mm_skinny", cb, (x, q) + tabs, {}, [((M, N), F16)]
        yield f"{cb}_mm_batched", cb, (x, q) + tabs, {}, [((M, N), F16)]
        yield f"decompress_{cb}_origorder", cb, (q,) + tabs, {}, [((N, K_IN), F16)]
    g = t(256, dtype=I64)
    q16 = CODEBOOKS["e8p"][0]
    qd4 = CODEBOOKS["d4"][0]
    q3 = CODEBOOKS["e8prvq3"][0]
    gd4 = t(256, 4)
    e81b_i8 = t(256, 8, dtype=I8)
    planes = t(PL, dtype=U8)
    q2 = t(2 * N, K_IN // 8, dtype=I16)
    vec = t(NP)
    x1 = t(1, NP)
    yield "hadamard", "", (t(M, 64), 0.5), {}, [((M, 64), F16)]
    yield "had_transform", "", (t(M, 1000), 1024, NP, 1, None, False, None, None, None, None, 1.0), {}, [((M, 1024), F16)]
    yield "had_transform_planes", "", (t(1, 1000), NP, 1, None, False, None, 1.0), {}, [((PL,), U8)]
    yield "had_transform_fused", "", (t(M, NP), 900, NP, 1, None, False, None, None, None, None, 1.0, None, None, 1e-5,
                                      None), {}, [((M, 900), F16)]
    yield "had_transform_planes_fused", "", (x1, NP, 1, None, False, None, 1.0, None, 1e-5, None), {}, [((PL,), U8)]
    yield "had_transform_planes_fused", "rvq", (x1, NP, 1, None, False, None, 1.0, None, 1e-5, None), \
        {"resid_scale": 0.5}, [((PL2,), U8)]
    yield "had_transform_planes_group", "", (x1, NP, 1, [None, None], False, [vec, vec], [1.0, 1.0], None, 1e-5, None), \
        {}, [((PL,), U8)] * 2
    yield "had_transform_planes_group", "hi", (x1, NP, 1, [None], False, [vec], [1.0], None, 1e-5, None), \
        {"resid_scale": register_lib.HI_PLANES}, [((PL2,), U8)]
    yield "had_transform_planes_rows", "", (t(M, NP), NP, 1, None, False, None, 1.0, None, 1e-5, None), {}, \
        [((M, PL), U8)]
    yield "had_transform_planes_rows", "rvq", (t(M, NP), NP, 1, None, False, None, 1.0, None, 1e-5, None), \
        {"resid_scale": 0.5}, [((M, PL2), U8)]
    yield "had_chain_planes_group", "", (x1, vec, None, 1.0, NP, [vec, vec, vec], [1.0, 1.0, 1.0], None, 1e-5), {}, \
        [((1, NP), F16)] + [((PL,), U8)] * 3
    yield "had_transform_group", "", ([t(M, NP), t(M, NP)], [512, 700], NP, 1, [None, None], False, [None, None],
                                      [None, None], [None, None], [1.0, 1.0], [None, None], [None, None], None, 1e-5), \
        {}, [((M, 512), F16), ((M, 700), F16)]
    yield "e8p_gemv_planes", "", (planes, q16, g), {}, [((1, N), F16)]
    yield "e8p_gemv_planes_group", "", ([planes, planes], [q16, q2], g), {}, [((1, N), F16), ((1, 2 * N), F16)]
    yield "d4_gemv_planes", "", (planes, qd4, gd4), {}, [((1, N), F16)]
    yield "d4_gemv_planes_group", "", ([planes, planes], [qd4, qd4], gd4), {}, [((1, N), F16)] * 2
    yield "e8prvq3_gemv_planes_group", "", ([planes], [q3], g, e81b_i8), {}, [((1, N), F16)]
    yield "e8p_mm_planes_rows", "", ([planes, planes], q16, g), {}, [((2, N), F16)]
    yield "e8p_gemv_planes_rows", "", (t(M, PL, dtype=U8), q16, g), {}, [((M, N), F16)]
    yield "gemv_planes_rows_mode", "d4", (t(M, PL, dtype=U8), qd4, gd4, None, 64), {}, [((M, N), F16)]
    yield "gemv_planes_rows_mode", "e8prvq3", (t(M, PL, dtype=U8), q3, g, e81b_i8, 40), {}, [((M, N), F16)]
    yield "e8p_gemv_fused", "x", (t(K_IN), None, None, None, None, 1e-5, 1.0, [t(K_IN)], [1.0], [q16], g), {}, \
        [((1, N), F16)]
    yield "e8p_gemv_fused", "z", (None, t(1, K_IN), t(K_IN), None, None, 1e-5, 1.0, [t(K_IN)] * 2, [1.0] * 2,
                                  [q16, q2], g), {}, [((1, K_IN), F16), ((1, N), F16), ((1, 2 * N), F16)]
    yield "e8p_quantize", "", (t(40, 8, dtype=F32), g), {}, [((40, 8), F32), ((40,), I64)]
    yield "argmax_step", "", (t(1, 100), t(1, dtype=I64), t(1, dtype=I64)), {}, None
    yield "ffn_engine", "", (planes, planes, t(64, 32, dtype=I16), t(64, 32, dtype=I16), t(256, 8, dtype=I16), t(100),
                             t(64), t(64), t(64), g, t(100, dtype=U8), 1.0, 1.0, 1), {}, [((1, 256), F16)]
    yield "block_engine", "", (t(256, dtype=U8), t(4096), t(1, dtype=I64), t(8, 128, dtype=F32), t(8, 128, dtype=F32),
                               g, t(64, dtype=U8), 1, 8, 1e-5, 0.1), {}, [((4096,), F16)]
    kc = t(4, 32, 64)
    yield "rope_attn_decode", "", (t(8, 64), t(4, 64), t(4, 64), t(32, 64, dtype=F32), t(32, 64, dtype=F32),
                                   t(1, dtype=I64), kc, kc), {"workspace": None}, [((8, 64), F16)]
    yield "rope_attn_decode_z", "", ([t(1, 512), t(1, 256), t(1, 256)], [t(512), t(256), t(256)], [1.0, 1.0, 1.0],
                                     t(32, 64, dtype=F32), t(32, 64, dtype=F32), t(1, dtype=I64), kc, kc), {}, \
        [((8, 64), F16)]


def test_every_op_has_a_pinned_fake():
    named = {c[0] for c in _calls()}
    assert named == set(register_lib._SCHEMAS)


def test_fakes_shapes_and_dtypes():
    for name, label, args, kwargs, want in _calls():
        out = getattr(torch.ops.quip_lib, name)(*args, **kwargs)
        if want is None:
            assert out is None, (name, label)
            continue
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        got = [(tuple(o.shape), o.dtype) for o in outs]
        assert all(o.device.type == "meta" for o in outs), (name, label)
        assert got == want, (name, label, got, want)
