"""The MLP half of a sparse-MoE decoder block (Mixtral) at decode rows, experts routed on the device.

quip_lib::moe_route_rows    RMSNorm, router logits, softmax, top-k, the sort "by expert, then by row" and the signed rows
quip_lib::mm_skinny_moe     the 1..2 products of the sorted rows against the stacked codes of the experts that own rows
quip_lib::moe_combine_rows  mode 1: SV of gate / up, SiLU product, SU of down; mode 0: SV of down, weighted sum, residual

QuantMoeMlp chains them with the existing Hadamard transform launches: nine launches per block whatever E is, nothing read
by the host in between, so a step captures into one graph that serves whatever experts later inputs select.
The ops are defined here, beside register_lib._SCHEMAS (the reference's op surface plus the inference path's), as the ops of
lora.py and score.py are."""
import ctypes
import math

import torch
from torch import nn

from . import capi
from . import register_lib as _R
from .qlinear import QuantLinear

MAX_ROWS, MAX_EXPERTS, MAX_TOP_K = 31, 64, 8      # kMoeMaxRows, kMoeMaxExperts, kMoeMaxTopK (csrc/moe_rows.hip.h)

try:
    _R._lib.define("moe_route_rows(Tensor h, Tensor ln_weight, Tensor router_weight, Tensor? su_gate, Tensor? su_up, "
                   "int top_k, int stacks, bool renorm, float eps) -> (Tensor, Tensor, Tensor, Tensor)")
    _R._lib.define("mm_skinny_moe(Tensor x, Tensor[] Qidxs, Tensor scale, Tensor start, int rows, int mode, Tensor grid) "
                   "-> Tensor")
    _R._lib.define("moe_combine_rows(Tensor t, Tensor? t2, Tensor? sv, Tensor? sv2, Tensor? su, Tensor? residual, "
                   "Tensor start, Tensor? pair_of, Tensor? weight, int top_k, int mode) -> Tensor")
    _DEFINED = True
except RuntimeError:
    _DEFINED = False


def _f16_on(what, name, t, dev, shape=None, optional=False):
    if t is None and optional:
        return
    _R._need(t is not None and t.dtype == torch.float16 and t.is_contiguous() and t.device == dev
             and (shape is None or tuple(t.shape) == tuple(shape)),
             f"{what}: {name} must be a contiguous float16 tensor" + (f" of shape {tuple(shape)}" if shape else "") +
             " on the input's device")


def _i32_on(what, name, t, dev, n, dtype=torch.int32):
    _R._need(t is not None and t.dtype == dtype and t.is_contiguous() and t.device == dev and tuple(t.shape) == (n,),
             f"{what}: {name} must be a contiguous {dtype} ({n},) tensor on the input's device")


def _moe_route_rows_cuda(h, ln_weight, router_weight, su_gate, su_up, top_k, stacks, renorm, eps):
    """h (M, hidden) fp16 -> xs (stacks, M top_k, hidden) fp16, start (E + 1) int32, pair_of (P) int32, weight (P) fp32"""
    what = "moe_route_rows"
    _R._need(h.is_cuda and h.dim() == 2 and h.dtype == torch.float16 and h.is_contiguous(),
             f"{what}: h must be a contiguous float16 (M, hidden) CUDA tensor")
    M, hidden = h.shape
    _R._need(router_weight.dim() == 2, f"{what}: router_weight must be (E, hidden)")
    E = router_weight.shape[0]
    _R._need(1 <= M <= MAX_ROWS and hidden % 8 == 0 and 1 <= E <= MAX_EXPERTS and 1 <= top_k <= min(E, MAX_TOP_K)
             and 1 <= stacks <= 2,
             f"{what}: M = {M} (1..{MAX_ROWS}), hidden = {hidden} (% 8), E = {E} (1..{MAX_EXPERTS}), top_k = {top_k} "
             f"(1..min(E, {MAX_TOP_K})), stacks = {stacks} (1..2)")
    _f16_on(what, "ln_weight", ln_weight, h.device, (hidden,))
    _f16_on(what, "router_weight", router_weight, h.device, (E, hidden))
    _f16_on(what, "su_gate", su_gate, h.device, (E, hidden), optional=True)
    _f16_on(what, "su_up", su_up, h.device, (E, hidden), optional=True)
    P = M * top_k
    xs = _R._empty((stacks, P, hidden), dtype=torch.float16, device=h.device)
    start = _R._empty((E + 1,), dtype=torch.int32, device=h.device)
    pair_of = _R._empty((P,), dtype=torch.int32, device=h.device)
    weight = _R._empty((P,), dtype=torch.float32, device=h.device)
    with torch.cuda.device(h.device):
        capi.check(capi.lib().quip_moe_route_rows_f16(
            h.data_ptr(), ln_weight.data_ptr(), router_weight.data_ptr(), _R._ptr(su_gate), _R._ptr(su_up), xs.data_ptr(),
            start.data_ptr(), pair_of.data_ptr(), weight.data_ptr(), M, hidden, E, int(top_k), int(stacks), int(bool(renorm)),
            float(eps), _R._stream(h)), "quip_moe_route_rows_f16")
    return xs, start, pair_of, weight


def mm_skinny_moe_supported(n, k):
    """the expert shapes quip_moe_mm_skinny_f16 takes: those of the single skinny launch"""
    return _R.e8p_mm_skinny_supported(1, n, k)


def _mm_skinny_moe_cuda(x, Qidxs, scale, start, rows, mode, grid):
    """x (G, P, k) fp16 sorted by expert, Qidxs[g] (E, n, k / 8) int16 -> (G, P, n) fp16; rows = the token count M"""
    what = "mm_skinny_moe"
    _R._need(mode == 0, f"{what}: mode {mode}: only 0 (e8p) is built; e8prvq4, d4, hi and e8prvq3 are refused")
    _R._need(x.is_cuda and x.dim() == 3 and x.dtype == torch.float16 and x.is_contiguous(),
             f"{what}: x must be a contiguous float16 (G, P, k) CUDA tensor")
    G, P, k = x.shape
    _R._need(1 <= G <= 2 and len(Qidxs) == G, f"{what}: x / Qidxs: 1..2 stacks, one code tensor per stack")
    q0 = Qidxs[0]
    _R._need(all(q.dim() == 3 and q.dtype == torch.int16 and q.is_contiguous() and q.device == x.device
                 and q.shape == q0.shape for q in Qidxs) and q0.shape[2] * 8 == k,
             f"{what}: Qidxs: contiguous int16 (E, n, k / 8) tensors of one shape on x's device, k = {k}")
    E, n = q0.shape[:2]
    _R._need(1 <= E <= MAX_EXPERTS and 1 <= rows <= MAX_ROWS and rows <= P <= rows * MAX_TOP_K,
             f"{what}: E = {E} (1..{MAX_EXPERTS}), rows = {rows} (1..{MAX_ROWS}), P = {P} (rows..{MAX_TOP_K} rows)")
    _R._need(mm_skinny_moe_supported(n, k), f"{what}: Qidxs: shape ({n}, {k}) needs {_R._SKINNY[1]}")
    _R._need(scale.dtype == torch.float32 and scale.is_contiguous() and scale.device == x.device
             and tuple(scale.shape) == (G, E), f"{what}: scale must be contiguous float32 (G, E) on x's device")
    _i32_on(what, "start", start, x.device, E + 1)
    (g,) = _R._CODEBOOKS["e8p"].tables(x, grid)
    y = _R._empty((G, P, n), dtype=torch.float16, device=x.device)
    with torch.cuda.device(x.device):
        capi.check(capi.lib().quip_moe_mm_skinny_f16(
            0, x.data_ptr(), (ctypes.c_void_p * G)(*[q.data_ptr() for q in Qidxs]), g.data_ptr(), scale.data_ptr(),
            start.data_ptr(), y.data_ptr(), G, E, int(rows), P, n, k, _R._stream(x)), "quip_moe_mm_skinny_f16")
    return y


def _moe_combine_rows_cuda(t, t2, sv, sv2, su, residual, start, pair_of, weight, top_k, mode):
    """mode 0: t (P, width) -> (P / top_k, width); mode 1: gate t, up t2 (P, width) -> (P, width)"""
    what = "moe_combine_rows"
    _R._need(mode in (0, 1), f"{what}: mode {mode}: 0 combine, 1 the SiLU product")
    _R._need(t.is_cuda and t.dim() == 2 and t.dtype == torch.float16 and t.is_contiguous(),
             f"{what}: t must be a contiguous float16 (P, width) CUDA tensor")
    P, width = t.shape
    E = start.numel() - 1
    _R._need(width % 8 == 0 and 1 <= E <= MAX_EXPERTS and 1 <= top_k <= min(E, MAX_TOP_K) and P % top_k == 0
             and 1 <= P // top_k <= MAX_ROWS,
             f"{what}: width = {width} (% 8), E = {E}, top_k = {top_k}, P = {P} (a multiple of top_k, at most {MAX_ROWS} rows)")
    _i32_on(what, "start", start, t.device, E + 1)
    for name, v in (("sv", sv), ("sv2", sv2), ("su", su)):
        _f16_on(what, name, v, t.device, (E, width), optional=True)
    if mode == 0:
        rows = P // top_k
        _R._need(t2 is None and sv2 is None and su is None, f"{what}: t2 / sv2 / su belong to mode 1")
        _i32_on(what, "pair_of", pair_of, t.device, P)
        _i32_on(what, "weight", weight, t.device, P, torch.float32)
        _f16_on(what, "residual", residual, t.device, (rows, width), optional=True)
    else:
        rows = P
        _R._need(residual is None, f"{what}: residual belongs to mode 0")
        _f16_on(what, "t2", t2, t.device, (P, width))
    out = _R._empty((rows, width), dtype=torch.float16, device=t.device)
    with torch.cuda.device(t.device):
        capi.check(capi.lib().quip_moe_combine_rows_f16(
            int(mode), t.data_ptr(), _R._ptr(t2), _R._ptr(sv), _R._ptr(sv2), _R._ptr(su), _R._ptr(residual), out.data_ptr(),
            start.data_ptr(), _R._ptr(pair_of), _R._ptr(weight), rows, width, E, int(top_k), P, _R._stream(t)),
            "quip_moe_combine_rows_f16")
    return out


if _DEFINED:
    _R._lib.impl("moe_route_rows", _moe_route_rows_cuda, "CUDA")
    _R._lib.impl("mm_skinny_moe", _mm_skinny_moe_cuda, "CUDA")
    _R._lib.impl("moe_combine_rows", _moe_combine_rows_cuda, "CUDA")
    _R._reg_fake("moe_route_rows", lambda h, ln_weight, router_weight, su_gate, su_up, top_k, stacks, renorm, eps: (
        h.new_empty((stacks, h.shape[0] * top_k, h.shape[1])),
        h.new_empty((router_weight.shape[0] + 1,), dtype=torch.int32),
        h.new_empty((h.shape[0] * top_k,), dtype=torch.int32),
        h.new_empty((h.shape[0] * top_k,), dtype=torch.float32)))
    _R._reg_fake("mm_skinny_moe", lambda x, Qidxs, scale, start, rows, mode, grid:
                 x.new_empty((x.shape[0], x.shape[1], Qidxs[0].shape[1])))
    _R._reg_fake("moe_combine_rows", lambda t, t2, sv, sv2, su, residual, start, pair_of, weight, top_k, mode:
                 t.new_empty((t.shape[0] // top_k if mode == 0 else t.shape[0], t.shape[1])))


# what the experts of one role (w1, w3 or w2) must share, checked on values; the first that differs is named
_SHARED = ("in_features", "out_features", "q_in_features", "q_out_features", "K_left", "K_right", "per_channel")


class QuantMoeMlp(nn.Module):
    """Router + E experts of three QuantLinear each (w1 gate, w3 up, w2 down: HF Mixtral's block_sparse_moe).

    All experts must share shape, codebook (E8P12), K_left / K_right and Hadamard factors, have no bias and a scalar
    Wscale; anything else is refused with the field's name.  Qidxs, SU, SV and the scales are stacked once; every module's
    Qidxs becomes a view of its slice of the stack, so residency does not double and every other path still reads the module.
    forward_rows serves 1..31 rows with the routed launches.  More rows (long prompt chunks) fall back to a loop over the
    experts on the existing ops, with the ids read by the host: that regime is not what this class is for."""

    def __init__(self, router_weight, experts, top_k, renorm=True):
        super().__init__()
        experts = [tuple(t) for t in experts]
        E = len(experts)
        if not (1 <= E <= MAX_EXPERTS and 1 <= top_k <= min(E, MAX_TOP_K)):
            raise NotImplementedError(f"n_experts = {E} (1..{MAX_EXPERTS}), top_k = {top_k} (1..min(n_experts, {MAX_TOP_K}))")
        if any(len(t) != 3 or not all(isinstance(m, QuantLinear) for m in t) for t in experts):
            raise TypeError("experts: (w1, w3, w2) triples of QuantLinear")
        self.top_k, self.renorm, self.n_experts = int(top_k), bool(renorm), E
        roles = {"w1": [t[0] for t in experts], "w3": [t[1] for t in experts], "w2": [t[2] for t in experts]}
        for role, mods in roles.items():
            self._check_role(role, mods)
        g0, u0, d0 = roles["w1"][0], roles["w3"][0], roles["w2"][0]
        for f in _SHARED:
            if getattr(g0, f) != getattr(u0, f):
                raise NotImplementedError(f"w1 and w3 differ in {f}: {getattr(g0, f)} != {getattr(u0, f)}")
        for f in ("had_left", "had_right"):
            if not self._same(getattr(g0, f), getattr(u0, f)):
                raise NotImplementedError(f"w1 and w3 differ in {f}")
        if d0.in_features != g0.out_features or d0.out_features != g0.in_features:
            raise NotImplementedError(f"w2 is ({d0.in_features} -> {d0.out_features}), w1 ({g0.in_features} -> {g0.out_features})")
        if tuple(router_weight.shape) != (E, g0.in_features):
            raise NotImplementedError(f"router weight {tuple(router_weight.shape)}, expected {(E, g0.in_features)}")
        self.experts = nn.ModuleList(nn.ModuleList(t) for t in experts)
        self.register_buffer("router", router_weight.detach().to(g0.Qidxs.device, torch.float16).contiguous())
        self.codebook = g0.codebook
        for role, mods in roles.items():
            q = torch.stack([m.Qidxs for m in mods]).contiguous()
            for i, m in enumerate(mods):
                m.Qidxs = q[i]
            self.register_buffer(f"q_{role}", q, persistent=False)
            for v in ("SU", "SV"):
                vs = [getattr(m, v) for m in mods]
                self.register_buffer(f"{v.lower()}_{role}", None if vs[0] is None else
                                     torch.stack([QuantLinear._vec(t) for t in vs]).contiguous(), persistent=False)
        dev = self.q_w1.device
        self.register_buffer("scale_gu", torch.tensor([[m.wscale_float for m in roles[r]] for r in ("w1", "w3")],
                                                      dtype=torch.float32, device=dev), persistent=False)
        self.register_buffer("scale_d", torch.tensor([[m.wscale_float for m in roles["w2"]]], dtype=torch.float32,
                                                     device=dev), persistent=False)

    def _apply(self, fn, *args, **kwargs):
        """a move (.to / .cuda / .half) copies the stacks and the modules' tensors one by one: afterwards every module's Qidxs is
        made a view of its slice of the moved stack again, so nothing is resident twice"""
        super()._apply(fn, *args, **kwargs)
        for j, role in enumerate(("w1", "w3", "w2")):
            q = getattr(self, f"q_{role}")
            for i, triple in enumerate(self.experts):
                triple[j].Qidxs = q[i]
        return self

    @staticmethod
    def _same(a, b):
        return (a is None and b is None) or (a is not None and b is not None and a.shape == b.shape and torch.equal(a, b))

    @classmethod
    def _check_role(cls, role, mods):
        m0 = mods[0]
        if getattr(m0.codebook, "id", None) != "E8P12":
            raise NotImplementedError(f"{role}: codebook {getattr(m0.codebook, 'id', None)!r}: the routed product serves E8P12")
        if m0.per_channel or m0.bias is not None:
            raise NotImplementedError(f"{role}: {'per_channel' if m0.per_channel else 'bias'} is not supported on routed experts")
        if m0.q_in_features % 128 != 0 or m0.q_out_features % 2 != 0:
            raise NotImplementedError(f"{role}: q_in_features {m0.q_in_features} % 128, q_out_features {m0.q_out_features} % 2")
        for i, m in enumerate(mods[1:], 1):
            if getattr(m.codebook, "id", None) != "E8P12":
                raise NotImplementedError(f"expert {i} {role} differs in codebook")
            for f in _SHARED:
                if getattr(m, f) != getattr(m0, f):
                    raise NotImplementedError(f"expert {i} {role} differs in {f}: {getattr(m, f)} != {getattr(m0, f)}")
            for f in ("had_left", "had_right"):
                if not cls._same(getattr(m, f), getattr(m0, f)):
                    raise NotImplementedError(f"expert {i} {role} differs in {f}")
            for f in ("SU", "SV", "bias"):
                if (getattr(m, f) is None) != (getattr(m0, f) is None):
                    raise NotImplementedError(f"expert {i} {role} differs in {f}: present on some experts only")
            if m.Qidxs.shape != m0.Qidxs.shape or m.Qidxs.dtype != m0.Qidxs.dtype or m.Qidxs.device != m0.Qidxs.device:
                raise NotImplementedError(f"expert {i} {role} differs in Qidxs")

    @classmethod
    def from_hf(cls, block_sparse_moe, top_k=None, renorm=True):
        """around HF Mixtral's block_sparse_moe: `gate.weight` (left unquantised, as the reference's README says) and
        `experts[i].w1 / w3 / w2`"""
        k = top_k if top_k is not None else getattr(block_sparse_moe, "top_k", None)
        if k is None:
            raise NotImplementedError("top_k: not given and the module has none")
        return cls(block_sparse_moe.gate.weight, [(e.w1, e.w3, e.w2) for e in block_sparse_moe.experts], int(k), renorm)

    @staticmethod
    def _transform(m, x, side):
        """the module's input (side 0) or output (side 1) Hadamard launch with no sign vector and no module scale"""
        if side == 0:
            n, K, had, out = m.q_in_features, m.K_left, m._had("had_left"), m.q_in_features
        else:
            n, K, had, out = m.q_out_features, m.K_right, m._had("had_right"), m.out_features
        return torch.ops.quip_lib.had_transform_fused(x, out, n, K, had, side == 0, None, None, None, None,
                                                      1.0 / math.sqrt(n // K), None, None, 1e-5, None)

    def forward_rows(self, h, ln_weight, eps):
        """h + moe(RMSNorm(h) * ln_weight) for h (M, hidden) fp16: nine launches for M <= 31, nothing read by the host"""
        M, hidden = h.shape
        if M > MAX_ROWS:
            return self._forward_loop(h, ln_weight, eps)
        ops, k = torch.ops.quip_lib, self.top_k
        g0, _, d0 = self.experts[0]
        P, grid = M * k, self.codebook.grid_packed_abs
        xs, start, pair_of, weight = ops.moe_route_rows(h, QuantLinear._vec(ln_weight), self.router, self.su_w1, self.su_w3,
                                                        k, 2, self.renorm, eps)
        xh = self._transform(g0, xs.view(2 * P, hidden), 0)
        z = ops.mm_skinny_moe(xh.view(2, P, -1), [self.q_w1, self.q_w3], self.scale_gu, start, M, 0, grid)
        t = self._transform(g0, z.view(2 * P, -1), 1)
        mid = ops.moe_combine_rows(t[:P], t[P:], self.sv_w1, self.sv_w3, self.su_w2, None, start, None, None, k, 1)
        xd = self._transform(d0, mid, 0)
        zd = ops.mm_skinny_moe(xd.view(1, P, -1), [self.q_w2], self.scale_d, start, M, 0, grid)
        td = self._transform(d0, zd.view(P, -1), 1)
        return ops.moe_combine_rows(td, None, self.sv_w2, None, None, h, start, pair_of, weight, k, 0)

    def _forward_loop(self, h, ln_weight, eps):
        """more than 31 rows: the router in torch, then every expert that owns rows on its own modules (ids on the host)"""
        x = h.float()
        xn = (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * ln_weight.float())
        logits = (xn @ self.router.float().T).to(torch.float16).float()
        # as the kernel: the top_k largest fp16 logits, the lower index on a tie (a stable sort), not the probabilities
        ids = torch.sort(logits, dim=-1, descending=True, stable=True).indices[:, :self.top_k]
        w = torch.softmax(logits, -1).gather(-1, ids)
        if self.renorm:
            w = w / w.sum(-1, keepdim=True)
        return self._experts_loop(h, ln_weight, eps, w, [(ids == e).nonzero(as_tuple=True) for e in range(self.n_experts)])

    def _experts_loop(self, h, ln_weight, eps, w, owned):
        """h + the weighted outputs of the experts; owned[e] = (rows, slots) of expert e, w (M, top_k) fp32"""
        out = h.float()
        for (w1, w3, w2), (rows, slots) in zip(self.experts, owned):
            if rows.numel():
                xe = h[rows].contiguous()
                y = w2.forward_fused(w3.forward_fused(xe, rms_weight=ln_weight, rms_eps=eps),
                                     gate=w1.forward_fused(xe, rms_weight=ln_weight, rms_eps=eps))
                out = out.index_add(0, rows, w[rows, slots, None] * y.float())
        return out.to(torch.float16)
