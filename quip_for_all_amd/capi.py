"""ctypes binding of libquip_mi355.so (include/quip_mi355.h).  This module is the
only place that touches the native library; it never falls back to a CPU path:
a missing library or symbol raises."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("QUIP_LIB_PATH") or os.path.join(_HERE, "lib", "libquip_mi355.so")   # override: debug builds

_c = ctypes
_P, _I32, _I64, _F = _c.c_void_p, _c.c_int32, _c.c_int64, _c.c_float

# name -> argtypes ; every entry of include/quip_mi355.h
SIGNATURES = {
    "quip_abi_version": [],
    "quip_device_cu_count": [],
    "quip_hadamard_f16": [_P, _P, _I64, _I32, _F, _P],
    "quip_hadamard": [_P, _P, _I64, _I32, _F, _I32, _P],
    "quip_had_transform_f16": [_P, _P, _I64, _I32, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _P, _F, _P],
    "quip_had_transform_planes": [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _F, _P],
    "quip_had_transform_fused_f16": [_P, _P, _I64, _I32, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _P, _F, _P, _P],
    "quip_had_transform_planes_fused": [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _F, _P, _P],
    "quip_had_transform_group_f16": [_P, _I32, _I64, _I32, _I32, _I32, _P],
    "quip_had_transform_planes_group": [_P, _I32, _I32, _I32, _I32, _P],
    "quip_e8p_gemv_planes_group": [_P, _P, _P, _P, _P, _I32, _I32, _P],
    "quip_e8p_gemv_workspace_bytes": [_I32],
    "quip_e8p_gemv_planes_ws": [_P, _P, _P, _P, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_e8p_gemv_planes_group_ws": [_P, _P, _P, _P, _P, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_had_transform_planes_rows": [_P, _I64, _I32, _I32, _I32, _P],
    "quip_e8p_gemv_max_rows": [_I32, _I32],
    "quip_e8p_quantize_f32": [_P, _I64, _P, _P, _P, _P],
    "quip_ldlq_panel_f32": [_P, _P, _P, _P, _I64, _I32, _P, _P, _P, _P],
    "quip_ldlq_panel_rvq_f32": [_P, _P, _P, _P, _I64, _I32, _P, _P, _F, _P, _P, _P],
    "quip_gemv_max_rows_mode": [_I32, _I32, _I32],
    "quip_gemv_planes_rows_mode": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P],
    "quip_e8p_gemv_planes_rows": [_P, _P, _P, _P, _I32, _I32, _I32, _P],
    "quip_e8prvq3_gemv_planes_group": [_P, _P, _P, _P, _P, _P, _I32, _I32, _P],
    "quip_e8prvq3_gemv_planes_group_ws": [_P, _P, _P, _P, _P, _P, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_d4_gemv_planes": [_P, _P, _P, _P, _I32, _I32, _P],
    "quip_d4_gemv_planes_group": [_P, _P, _P, _P, _P, _I32, _I32, _P],
    "quip_d4_gemv_planes_v2": [_P, _P, _P, _P, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_d4_gemv_planes_group_ws": [_P, _P, _P, _P, _P, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_e8p_gemv_fused": [_P, _P, _P, _P, _P, _I32, _I32, _P],
    "quip_rope_attn_workspace_bytes": [_I32, _I32],
    "quip_argmax_step_f16": [_P, _I32, _P, _P, _P],
    "quip_rope_attn_decode_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P],
    "quip_rope_attn_decode_window_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, _P],
    "quip_rope_attn_decode_z_window_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, _P],
    "quip_rope_attn_decode_z_supported": [_I32, _I32, _I32],
    "quip_rope_attn_decode_z_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _P, _P],
    "quip_rope_attn_batched_workspace_bytes": [_I32, _I32, _I32],
    "quip_rope_attn_decode_batched_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _I32,
                                          _P, _P],
    "quip_rope_attn_decode_batched_start_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F,
                                                _I32, _P, _P, _P],
    "quip_argmax_step_batched_f16": [_P, _I32, _I32, _P, _P, _P],
    "quip_rope_attn_chunk_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P],
    "quip_rope_attn_ragged_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _F,
                                  _I32, _P],
    "quip_rope_attn_decode_paged_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32,
                                        _F, _I32, _P, _P],
    "quip_rope_attn_ragged_paged_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32,
                                        _I32, _P, _P, _I32, _F, _I32, _P],
    "quip_rope_attn_decode_paged_f8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32,
                                       _F, _I32, _P, _P, _I32, _I32],
    "quip_rope_attn_ragged_paged_f8": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32,
                                       _I32, _P, _P, _I32, _F, _I32, _P, _I32, _I32],
    "quip_nll_rows_f16": [_P, _I32, _I32, _P, _P, _P, _P, _P],
    "quip_sample_step_f16": [_P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _P],
    "quip_spec_draft_i64": [_P, _P, _P, _P, _I32, _P, _P, _I32, _P, _I32, _I32, _I32, _P],
    "quip_spec_accept_draft_i64": [_P, _P, _P, _P, _P, _P, _I32, _P, _P, _I32, _P, _P, _I32, _P, _I32, _I32, _I32, _P],
    "quip_qk_norm_rows_f16": [_P, _P, _P, _P, _I64, _I32, _I32, _I32, _F, _P],
    "quip_rope_attn_decode_qknorm_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _F, _I32, _P, _P,
                                         _P, _P, _F],
    "quip_rope_attn_decode_batched_qknorm_f16": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _F,
                                                 _I32, _P, _P, _P, _P, _F],
    "quip_lora_shrink_rows_f16": [_P, _P, _P, _P, _I64, _I32, _I32, _I32, _I32, _P, _F, _P],
    "quip_lora_expand_rows_f16": [_P, _P, _P, _I64, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P],
    "quip_block_engine_supported": [_I32, _I32, _I32, _I32, _I32, _I32],
    "quip_block_engine_workspace_bytes": [],
    "quip_block_engine_layer_bytes": [],
    "quip_block_engine": [_P, _P],
    "quip_block_engine_token": [_P, _P, _P],
    "quip_debug_occupy": [_I32, _I32, _c.c_int64, _P, _P],
    "quip_block_engine_gqa_supported": [_I32, _I32, _I32, _I32, _I32, _I32],
    "quip_block_engine_gqa_workspace_bytes": [],
    "quip_block_engine_g8_supported": [_I32, _I32, _I32, _I32, _I32, _I32],
    "quip_block_engine_g8_workspace_bytes": [],
    "quip_e8p_gemv_kernel_choice": [_P, _I32, _I32],
    "quip_ffn_engine_supported": [_I32, _I32, _I32],
    "quip_ffn_engine_workspace_bytes": [_I32, _I32],
    "quip_ffn_engine": [_P, _P],
    "quip_tile_codes": [_P, _P, _I64, _I64, _P],
    "quip_untile_codes": [_P, _P, _I64, _I64, _P],
    "quip_tile_codes_view": [_P, _P, _I64, _I64, _P],
    "quip_untile_codes_view": [_P, _P, _I64, _I64, _P],
    "quip_e8p_mm_origorder": [_P, _P, _P, _P, _I32, _I32, _I32, _P],
    "quip_e8p_mm_batched": [_P, _P, _P, _P, _I64, _I32, _I32, _P],
    "quip_e8prvq4_mm_batched": [_P, _P, _P, _F, _P, _I64, _I32, _I32, _P],
    "quip_e8prvq3_mm_batched": [_P, _P, _P, _P, _F, _P, _I64, _I32, _I32, _P],
    "quip_d4_mm_batched": [_P, _P, _P, _P, _I64, _I32, _I32, _P],
    "quip_hi_mm_batched": [_P, _P, _P, _I64, _I32, _I32, _P],
    "quip_e8p_mm_skinny": [_P, _P, _P, _P, _I32, _I32, _I32, _P],
    "quip_e8prvq4_mm_skinny": [_P, _P, _P, _F, _P, _I32, _I32, _I32, _P],
    "quip_e8prvq3_mm_skinny": [_P, _P, _P, _P, _F, _P, _I32, _I32, _I32, _P],
    "quip_d4_mm_skinny": [_P, _P, _P, _P, _I32, _I32, _I32, _P],
    "quip_hi_mm_skinny": [_P, _P, _P, _I32, _I32, _I32, _P],
    "quip_e8p_mm_workspace_bytes": [_I32, _I32, _I32],
    "quip_e8p_mm_origorder_ws": [_P, _P, _P, _P, _I32, _I32, _I32, _P, _c.c_size_t, _P],
    "quip_e8p_planes_bytes": [_I32],
    "quip_e8p_x_to_planes": [_P, _P, _I32, _P],
    "quip_e8p_gemv_planes": [_P, _P, _P, _P, _I32, _I32, _P],
    "quip_e8prvq3_mm_origorder": [_P, _P, _P, _P, _F, _P, _I32, _I32, _I32, _P],
    "quip_e8prvq4_mm_origorder": [_P, _P, _P, _F, _P, _I32, _I32, _I32, _P],
    "quip_d4_mm_origorder": [_P, _P, _P, _P, _I32, _I32, _I32, _P],
    "quip_hi_mm_origorder": [_P, _P, _P, _I32, _I32, _I32, _P],
    "quip_decompress_e8p_origorder": [_P, _P, _P, _I64, _I32, _P],
    "quip_decompress_e8prvq3_origorder": [_P, _P, _P, _F, _P, _I64, _I32, _P],
    "quip_decompress_e8prvq4_origorder": [_P, _P, _F, _P, _I64, _I32, _P],
    "quip_decompress_d4_origorder": [_P, _P, _P, _I64, _I32, _P],
    "quip_decompress_hi_origorder": [_P, _P, _I64, _I32, _P],
}
# not part of the public header: tuning hook used by the micro-benchmarks only
_INTERNAL = {
    "quip_e8p_x_to_planes_laneorder": [_P, _P, _I32, _P],
    "quip_e8p_gemv_fused_tuned": [_P, _P, _P, _P, _P, _I32, _I32, _P, _P],
    "quip_e8p_gemv_group_tuned": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P],
    "quip_e8p_gemv_v2_tuned": [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P],
    "quip_e8p_gemv_v2_group_tuned": [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P],
    "quip_e8p_gemv_v2_workspace_bytes": [_I32],
    "quip_e8p_gemv_v2_plan": [_P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P],
    "quip_e8p_gemv_tuned": [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P],
    "quip_had_plan": [_P, _I32, _I32, _I64, _I32, _I32, _I32, _P],
}

class HadProblem(_c.Structure):
    """mirror of quip_had_problem (include/quip_mi355.h)"""
    _fields_ = [("x", _P), ("out", _P), ("had", _P), ("pre_scale", _P), ("pre_scale2", _P), ("post_scale", _P),
                ("bias", _P), ("residual", _P), ("rms_weight", _P), ("gate", _P), ("in_features", _I32),
                ("out_features", _I32), ("scale", _F), ("rms_eps", _F),
                ("z", _P), ("z_post_scale", _P), ("z_residual", _P), ("h_out", _P), ("z_scale", _F),
                ("resid_scale", _F), ("planes_layout", _I32), ("n", _I32), ("z_had", _P)]


MAX_GROUP = 3


class GemvFusedIn(_c.Structure):
    """mirror of quip_gemv_fused_in (include/quip_mi355.h)"""
    _fields_ = [("x", _P), ("z", _P), ("post_scale", _P), ("residual", _P), ("h_out", _P), ("rms_weight", _P),
                ("pre_scale", _P * 3), ("scale", _F * 3), ("z_scale", _F), ("rms_eps", _F)]


class FfnEngineArgs(_c.Structure):
    """mirror of quip_ffn_engine_args (include/quip_mi355.h)"""
    _fields_ = [("w_gate", _P), ("w_up", _P), ("w_down", _P), ("planes_gate", _P), ("planes_up", _P), ("had3", _P),
                ("sv_gate", _P), ("sv_up", _P), ("su_down", _P), ("z_down", _P), ("grid_packed_abs", _P),
                ("workspace", _P), ("dbg", _P), ("out_scale", _F), ("in_scale", _F), ("hidden", _I32),
                ("n_ffn", _I32), ("K", _I32)]


class BlockEngineArgs(_c.Structure):
    """mirror of quip_block_engine_args (include/quip_mi355.h)"""
    _fields_ = [("layers", _P), ("h_in", _P), ("h_out", _P), ("pos", _P), ("cos", _P), ("sin", _P),
                ("grid_packed_abs", _P), ("workspace", _P), ("dbg", _P), ("n_layers", _I32), ("max_len", _I32),
                ("dbg_layer", _I32), ("rms_eps", _F), ("attn_scale", _F), ("codebook", _I32), ("resid_scale", _F),
                ("shape", _I32), ("grid2", _P)]


class TokenTailArgs(_c.Structure):
    """mirror of quip_token_tail_args (include/quip_mi355.h)"""
    _fields_ = [("tok", _P), ("pos", _P), ("embed", _P), ("final_norm", _P), ("lm_head", _P), ("logits", _P),
                ("xnorm", _P), ("vocab", _I32)]


class HadFusion(_c.Structure):
    """mirror of quip_had_fusion (include/quip_mi355.h)"""
    _fields_ = [("residual", _P), ("rms_weight", _P), ("gate", _P), ("rms_eps", _F)]


_lib = None


class QuipNativeError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise QuipNativeError(
                f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, args in list(SIGNATURES.items()) + list(_INTERNAL.items()):
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.argtypes = args
            fn.restype = _c.c_size_t if name.endswith("_bytes") else _c.c_int
        L.quip_strerror.argtypes = [_c.c_int]
        L.quip_strerror.restype = _c.c_char_p
        L.quip_had_plan_kind_name.argtypes = [_I32]
        L.quip_had_plan_kind_name.restype = _c.c_char_p
        _lib = L
    return _lib


def check_symbols():
    L = lib()
    missing = [n for n in list(SIGNATURES) + ["quip_strerror"] if not hasattr(L, n)]
    if missing:
        raise QuipNativeError(f"libquip_mi355.so lacks symbols: {missing}")
    return sorted(SIGNATURES) + ["quip_strerror"]


GEMV_V2_PLAN_FIELDS = ("rc", "rep", "slots", "ksplit", "nrb", "spw", "rpb0", "rpb1", "rpb2", "runlen", "rpr_inv", "threads",
                       "lds")


def gemv_v2_plan(ns, k, rep=0, slots=0, blocks=0, ksplit=0, max_waves=0, runlen=0, grid2=False, ws=True):
    """The launch plan of the K-splitting GEMV for these tuning arguments (rep 4: nibble mode) as a list in the order of
    GEMV_V2_PLAN_FIELDS.  Host arithmetic only: nothing is launched, no GPU is needed."""
    n = (_I32 * max(len(ns), 1))(*ns)
    out = (_I32 * len(GEMV_V2_PLAN_FIELDS))()
    lib().quip_e8p_gemv_v2_plan(n, len(ns), k, rep, slots, blocks, ksplit, max_waves, runlen, int(bool(grid2)), int(bool(ws)), out)
    return list(out)


HAD_PLAN_FIELDS = ("rc", "kind", "grid_x", "grid_y", "grid_z", "threads", "lds")
HAD_PLAN_PROBLEM_FIELDS = ("pp", "tgroups", "part_off", "chain_off", "vec", "vec_out")


def had_plan(problems, planes, rows, n, K, transpose=0):
    """The plan of the transform launch that quip_had_transform_group_f16 (planes false) / _planes_group and _planes_rows
    (planes true) would make for these HadProblems: [rc, kernel instantiation as text or None, grid x, y, z, threads, lds,
    then one list in the order of HAD_PLAN_PROBLEM_FIELDS per problem].  The entry point's validation runs, nothing is
    launched and no pointer is dereferenced: host scratch pointers do, no GPU is needed."""
    arr = (HadProblem * max(len(problems), 1))(*problems)
    out = (_I32 * (len(HAD_PLAN_FIELDS) + len(HAD_PLAN_PROBLEM_FIELDS) * MAX_GROUP))()
    lib().quip_had_plan(arr, len(problems), int(bool(planes)), rows, n, K, transpose, out)
    v, name = list(out), lib().quip_had_plan_kind_name(out[1])
    per = [v[7 + 6 * i:13 + 6 * i] for i in range(v[4])]
    return [v[0], name.decode() if name else None] + v[2:7] + per


def had_plan_kinds():
    """every kernel instantiation a transform launch can take, as text, in the order of the library's enum"""
    names, L = [], lib()
    while L.quip_had_plan_kind_name(len(names)):
        names.append(L.quip_had_plan_kind_name(len(names)).decode())
    return names


def check(code, what):
    if code != 0:
        msg = lib().quip_strerror(code).decode()
        raise QuipNativeError(f"{what} failed: {msg} ({code})")
