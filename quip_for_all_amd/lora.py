"""LoRA adapters on the quantised decoders: a side branch beside every QuantLinear, one adapter index per row.

A QuIP# weight exists only as lattice codes behind two Hadamard transforms, so W + BA has no code: an adapter trained on
such a checkpoint runs beside the base module for good.  Two launches carry it (csrc/lora_rows.hip.h):

quip_lib::lora_shrink_rows   t[row] = A[a] xin(row), a = row_adapter[row]; xin is the input the base module sees -- x, the
                             RMSNorm that rides on the module's Hadamard launch, or x * silu(gate) -- in fp32
quip_lib::lora_expand_rows   y_j[row] = fp16(y_j[row] + scale[a, j] B_j[a] t[row, r0_j : r0_j + R_j]) for the 1..3 modules
                             that share the input, in place

Both are row-wise (a row's bits depend on its own inputs, its adapter index and that adapter's weights only) with a fixed
order of additions: chunked, ragged, paged and batched passes keep identical bits.  A negative index means no adapter:
zeros from the shrink, nothing written by the expand.

`LoraState` (LlamaDecoder.enable_lora) owns, per block and per input group (q/k/v, o, gate/up, down), the stacked A, B and
scale tensors of `max_adapters` adapter slots: allocated once at fixed addresses, zero-filled, ranks padded to a multiple of
8 -- a captured step survives loading, unloading and switching adapters.  Adapters come in PEFT's key scheme
(`read_peft_dir`; peft itself is not needed).  `shrink_ref` / `expand_ref` are the float64 statements the tests check
against."""
import json
import math
import os
import re

import numpy as np
import torch

from . import capi
from . import register_lib as _R

MAX_IN, MAX_RANK = 28672, 192                      # the shrink launch's limits (csrc/lora_rows.hip.h)
GROUPS = {"qkv": ("q", "k", "v"), "o": ("o",), "gu": ("gate", "up"), "down": ("down",)}
PEFT_MODULES = {"q_proj": "q", "k_proj": "k", "v_proj": "v", "o_proj": "o", "gate_proj": "gate", "up_proj": "up",
                "down_proj": "down"}
_KEY = re.compile(r"layers\.(\d+)\.(?:self_attn|mlp)\.(\w+)\.lora_([AB])(?:\.[^.]+)?\.weight$")

try:
    _R._lib.define("lora_shrink_rows(Tensor x, Tensor A, Tensor row_adapter, Tensor? rms_weight=None, float rms_eps=1e-5, "
                   "Tensor? gate=None) -> Tensor")
    _R._lib.define("lora_expand_rows(Tensor t, Tensor(a!)[] ys, Tensor[] Bs, Tensor scale, Tensor row_adapter, int[] r0) -> ()")
except RuntimeError:
    pass


def _check_rows(what, x, row_adapter):
    need = _R._need
    need(x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.shape[0] >= 1, f"{what}: a contiguous (rows, n) CUDA tensor")
    need(row_adapter.dtype == torch.int32 and row_adapter.is_contiguous() and row_adapter.device == x.device
         and tuple(row_adapter.shape) == (x.shape[0],), f"{what}: row_adapter must be a contiguous int32 (rows,) tensor on "
         "the rows' device")


def _lora_shrink_rows_cuda(x, A, row_adapter, rms_weight=None, rms_eps=1e-5, gate=None):
    """x (rows, in) fp16, A (n_adapters, R, in) fp16, row_adapter (rows,) int32 -> t (rows, R) fp32"""
    need = _R._need
    need(x.dtype == torch.float16, "lora_shrink_rows: x must be float16")
    _check_rows("lora_shrink_rows", x, row_adapter)
    rows, n_in = x.shape
    need(A.dtype == torch.float16 and A.dim() == 3 and A.is_contiguous() and A.device == x.device and A.shape[0] >= 1
         and A.shape[2] == n_in, "lora_shrink_rows: A must be contiguous float16 (n_adapters, R, in) on x's device")
    R = A.shape[1]
    need(n_in % 8 == 0 and 8 <= n_in <= MAX_IN, f"lora_shrink_rows: in = {n_in} (a multiple of 8 in 8 .. {MAX_IN})")
    need(R % 8 == 0 and 8 <= R <= MAX_RANK, f"lora_shrink_rows: R = {R} (a multiple of 8 in 8 .. {MAX_RANK})")
    need(rms_weight is None or gate is None, "lora_shrink_rows: rms_weight or gate, not both")
    mode, aux = 0, None
    if rms_weight is not None:
        need(rms_weight.dtype == torch.float16 and rms_weight.is_contiguous() and rms_weight.device == x.device
             and tuple(rms_weight.shape) == (n_in,), "lora_shrink_rows: rms_weight must be contiguous float16 (in,)")
        mode, aux = 1, rms_weight
    if gate is not None:
        need(gate.dtype == torch.float16 and gate.is_contiguous() and gate.device == x.device
             and tuple(gate.shape) == (rows, n_in), "lora_shrink_rows: gate must be contiguous float16 with x's shape")
        mode, aux = 2, gate
    t = torch.empty(rows, R, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        capi.check(capi.lib().quip_lora_shrink_rows_f16(x.data_ptr(), A.data_ptr(), row_adapter.data_ptr(), t.data_ptr(), rows,
                                                        n_in, R, A.shape[0], mode, _R._ptr(aux), float(rms_eps), _R._stream(x)),
                   "quip_lora_shrink_rows_f16")
    return t


def _lora_expand_rows_cuda(t, ys, Bs, scale, row_adapter, r0):
    """t (rows, R) fp32; ys[j] (rows, out_j) fp16, updated in place; Bs[j] (n_adapters, out_j, R_j) fp16; scale
    (n_adapters, 3) fp32; r0[j]: where module j's ranks begin in t.  out_j = 0 skips segment j."""
    need = _R._need
    need(t.dtype == torch.float32, "lora_expand_rows: t must be float32")
    _check_rows("lora_expand_rows", t, row_adapter)
    rows, Rt = t.shape
    nseg = len(ys)
    need(1 <= nseg <= 3 and len(Bs) == nseg and len(r0) == nseg, "lora_expand_rows: 1 .. 3 segments, as many Bs and r0")
    need(Rt % 8 == 0 and 8 <= Rt <= MAX_RANK, f"lora_expand_rows: t has {Rt} ranks (a multiple of 8 in 8 .. {MAX_RANK})")
    n = Bs[0].shape[0] if Bs[0].dim() == 3 else 0
    need(scale.dtype == torch.float32 and scale.is_contiguous() and scale.device == t.device
         and tuple(scale.shape) == (n, 3) and n >= 1, "lora_expand_rows: scale must be contiguous float32 (n_adapters, 3)")
    outs, Rs = [], []
    for j, (y, B) in enumerate(zip(ys, Bs)):
        need(y.dtype == torch.float16 and y.dim() == 2 and y.is_contiguous() and y.device == t.device and y.shape[0] == rows,
             "lora_expand_rows: ys must be contiguous float16 (rows, out_j) on t's device")
        need(B.dtype == torch.float16 and B.dim() == 3 and B.device == t.device and B.shape[0] == n
             and B.shape[1] == y.shape[1] and (B.is_contiguous() or B.numel() == 0),
             "lora_expand_rows: Bs must be contiguous float16 (n_adapters, out_j, R_j) on t's device")
        Rj, o = B.shape[2], y.shape[1]
        need(o % 8 == 0, f"lora_expand_rows: out_{j} = {o} (a multiple of 8)")
        need(Rj % 8 == 0 and Rj >= 8 and int(r0[j]) >= 0 and int(r0[j]) % 8 == 0 and int(r0[j]) + Rj <= Rt,
             f"lora_expand_rows: segment {j}: ranks [{int(r0[j])}, {int(r0[j]) + Rj}) of {Rt} (multiples of 8)")
        outs.append(o)
        Rs.append(Rj)
    P3, I3 = capi._P * 3, capi._I32 * 3
    pad = [0] * (3 - nseg)
    yp = P3(*[y.data_ptr() if y.numel() else None for y in ys] + [None] * (3 - nseg))
    bp = P3(*[B.data_ptr() if B.numel() else None for B in Bs] + [None] * (3 - nseg))
    with torch.cuda.device(t.device):
        capi.check(capi.lib().quip_lora_expand_rows_f16(t.data_ptr(), row_adapter.data_ptr(), scale.data_ptr(), rows, Rt, n,
                                                        nseg, yp, bp, I3(*outs + pad), I3(*Rs + pad),
                                                        I3(*[int(v) for v in r0] + pad), _R._stream(t)),
                   "quip_lora_expand_rows_f16")


try:
    _R._lib.impl("lora_shrink_rows", _lora_shrink_rows_cuda, "CUDA")
    _R._lib.impl("lora_expand_rows", _lora_expand_rows_cuda, "CUDA")
    _R._reg_fake("lora_shrink_rows", lambda x, A, row_adapter, rms_weight=None, rms_eps=1e-5, gate=None:
                 x.new_empty((x.shape[0], A.shape[1]), dtype=torch.float32))
    _R._reg_fake("lora_expand_rows", lambda t, ys, Bs, scale, row_adapter, r0: None)
except RuntimeError:
    pass


# ---- adapters in PEFT's file and key scheme ---------------------------------------------------------------------------------
def check_config(config, max_rank):
    """what of a PEFT LoraConfig (a dict: adapter_config.json) is served -> (r, scale, targets as module names of
    decode.PROJECTIONS).  Everything that would change the arithmetic and is not built is refused, naming the field."""
    c = dict(config)

    def refuse(field, why):
        raise NotImplementedError(f"adapter config: {field} {why}")
    if c.get("peft_type", "LORA") not in ("LORA", None):
        refuse("peft_type", f"= {c['peft_type']!r}: only LORA")
    if c.get("use_dora"):
        refuse("use_dora", "is set: DoRA is not built")
    if c.get("bias", "none") not in ("none", None):
        refuse("bias", f"= {c['bias']!r}: only 'none'")
    if c.get("modules_to_save"):
        refuse("modules_to_save", f"= {c['modules_to_save']!r}: trained copies of base modules are not served")
    for f in ("rank_pattern", "alpha_pattern"):
        if c.get(f):
            refuse(f, f"= {c[f]!r}: one r and one lora_alpha for all modules")
    if c.get("fan_in_fan_out"):
        refuse("fan_in_fan_out", "is set: the weights would be transposed")
    r = c.get("r")
    if isinstance(r, bool) or not isinstance(r, int) or r < 1:
        refuse("r", f"= {r!r}: a positive integer")
    if r > int(max_rank):
        refuse("r", f"= {r} exceeds max_rank = {int(max_rank)} of enable_lora")
    tm = c.get("target_modules")
    tm = [tm] if isinstance(tm, str) else list(tm or [])
    bad = [m for m in tm if m not in PEFT_MODULES]
    if not tm or bad:
        refuse("target_modules", f"= {tm!r}: a non-empty subset of {sorted(PEFT_MODULES)}")
    alpha = float(c.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if c.get("use_rslora") else alpha / r
    return r, scale, sorted({PEFT_MODULES[m] for m in tm}, key=list(PEFT_MODULES.values()).index)


def read_peft_dir(path):
    """(tensors, config) of a directory as PEFT's save_pretrained writes it: adapter_config.json plus
    adapter_model.safetensors or adapter_model.bin"""
    with open(os.path.join(path, "adapter_config.json")) as f:
        config = json.load(f)
    st = os.path.join(path, "adapter_model.safetensors")
    if os.path.exists(st):
        from safetensors.torch import load_file
        return load_file(st), config
    pt = os.path.join(path, "adapter_model.bin")
    if not os.path.exists(pt):
        raise FileNotFoundError(f"{path}: neither adapter_model.safetensors nor adapter_model.bin")
    return torch.load(pt, map_location="cpu", weights_only=True), config


def parse_tensors(tensors, n_layers, r, targets, dims):
    """PEFT keys (`...layers.{i}.self_attn.q_proj.lora_A.weight` (r, in), `lora_B.weight` (out, r)) -> {(layer, module):
    [A, B]}; dims: module -> (in, out).  Every target needs both matrices in every layer, nothing else may be there and the
    shapes must be the model's."""
    got = {}
    for key, w in tensors.items():
        m = _KEY.search(key)
        if m is None or m.group(2) not in PEFT_MODULES:
            raise ValueError(f"adapter tensors: {key!r} is not a lora_A / lora_B weight of one of {sorted(PEFT_MODULES)}")
        i, mod, ab = int(m.group(1)), PEFT_MODULES[m.group(2)], m.group(3)
        if mod not in targets:
            raise ValueError(f"adapter tensors: {key!r} is outside target_modules")
        if not 0 <= i < n_layers:
            raise ValueError(f"adapter tensors: {key!r}: the model has {n_layers} layers")
        n_in, n_out = dims[mod]
        want = (r, n_in) if ab == "A" else (n_out, r)
        if tuple(w.shape) != want:
            raise ValueError(f"adapter tensors: {key!r} has shape {tuple(w.shape)}, the model needs {want}")
        got.setdefault((i, mod), [None, None])[0 if ab == "A" else 1] = w
    for i in range(n_layers):
        for mod in targets:
            if (i, mod) not in got or any(w is None for w in got[(i, mod)]):
                raise ValueError(f"adapter tensors: lora_A / lora_B of layer {i}, module {mod!r} missing")
    return got


class LoraLayer:
    """the stacks of one decoder block: per group A (n, modules * Rp, in), per module B (n, out, Rp), scale (n, 3) shared"""

    def __init__(self, state, L):
        n, Rp, dev = state.max_adapters, state.rank, state.dev
        self.state = state
        self.A, self.B = {}, {}
        for g, mods in GROUPS.items():
            n_in = L[mods[0]].in_features
            if n_in % 8 or not 8 <= n_in <= MAX_IN or len(mods) * Rp > MAX_RANK or any(L[m].out_features % 8 for m in mods):
                raise NotImplementedError(f"LoRA on {mods}: in = {n_in}, {len(mods)} x {Rp} ranks (in: a multiple of 8 up to "
                                          f"{MAX_IN}; stacked ranks up to {MAX_RANK}; out: a multiple of 8)")
            self.A[g] = torch.zeros(n, len(mods) * Rp, n_in, dtype=torch.float16, device=dev)
            for m in mods:
                self.B[m] = torch.zeros(n, L[m].out_features, Rp, dtype=torch.float16, device=dev)

    def shrink(self, group, x, adapter, rms_weight=None, rms_eps=1e-5, gate=None):
        """t (rows, modules * Rp) fp32 of the group's stacked ranks, or None when no loaded adapter targets the group"""
        if not any(self.state.active(m) for m in GROUPS[group]):
            return None
        x = x.reshape(-1, x.shape[-1])
        return torch.ops.quip_lib.lora_shrink_rows(x, self.A[group], adapter, rms_weight, rms_eps,
                                                   None if gate is None else gate.reshape(x.shape))

    def expand(self, group, t, ys, adapter):
        """ys (the outputs of the group's modules, or the residual in front of o / down) += scale B t, in place; modules no
        loaded adapter targets are skipped"""
        Rp, ys2, Bs = self.state.rank, [], []
        for m, y in zip(GROUPS[group], ys):
            y2 = y.view(-1, y.shape[-1])
            on = self.state.active(m)
            ys2.append(y2 if on else y2[:, :0])
            Bs.append(self.B[m] if on else self.B[m][:, :0])
        torch.ops.quip_lib.lora_expand_rows(t, ys2, Bs, self.state.scale, adapter, [j * Rp for j in range(len(ys2))])
        return ys


class LoraState:
    """the adapter slots of one LlamaDecoder (enable_lora): registry, stacks, and the bs = 1 adapter index"""

    def __init__(self, dec, max_adapters=4, max_rank=16):
        max_adapters, max_rank = int(max_adapters), int(max_rank)
        if max_adapters < 1 or max_rank < 1:
            raise ValueError(f"enable_lora: max_adapters {max_adapters}, max_rank {max_rank} (both >= 1)")
        self.max_adapters, self.max_rank, self.rank = max_adapters, max_rank, (max_rank + 7) // 8 * 8
        self.dev = dec.dev
        self.n_layers = len(dec.layers)
        self.dims = {m: (dec.layers[0][m].in_features, dec.layers[0][m].out_features)
                     for mods in GROUPS.values() for m in mods}
        self.names = [None] * max_adapters            # slot -> name
        self.targets = [()] * max_adapters            # slot -> targeted modules
        self.scale = torch.zeros(max_adapters, 3, dtype=torch.float32, device=self.dev)
        self.idx = torch.full((1,), -1, dtype=torch.int32, device=self.dev)      # the bs = 1 step's adapter, read in place
        self.layers = [LoraLayer(self, L) for L in dec.layers]
        self.on_launches_changed = lambda: None       # (the decoder drops its captured steps)

    def active(self, module):
        return any(module in t for t in self.targets)

    def index(self, name):
        """slot of a loaded adapter; None -> -1 (no adapter)"""
        if name is None:
            return -1
        if name not in self.names:
            raise KeyError(f"adapter {name!r} is not loaded (loaded: {[n for n in self.names if n is not None]})")
        return self.names.index(name)

    def bytes_per_slot(self):
        """device bytes one adapter slot holds over all blocks"""
        one = self.layers[0]
        return self.n_layers * 2 * (sum(a[0].numel() for a in one.A.values()) + sum(b[0].numel() for b in one.B.values()))

    def load(self, name, tensors, config):
        """validate everything, then write the adapter into a slot (its own when the name is loaded already, else the first
        free one) -> the slot"""
        if not isinstance(name, str) or not name:
            raise ValueError("load_adapter: a non-empty name")
        r, scale, targets = check_config(config, self.max_rank)
        got = parse_tensors(tensors, self.n_layers, r, targets, self.dims)
        if name in self.names:
            slot = self.names.index(name)
        elif None in self.names:
            slot = self.names.index(None)
        else:
            raise RuntimeError(f"load_adapter: all max_adapters = {self.max_adapters} slots are taken ({self.names}); "
                               "unload one first")
        before = {m for t in self.targets for m in t}
        Rp = self.rank
        with torch.no_grad():
            self._zero(slot)
            for (i, mod), (A, B) in got.items():
                g, j = next((g, mods.index(mod)) for g, mods in GROUPS.items() if mod in mods)
                self.layers[i].A[g][slot, j * Rp:j * Rp + r].copy_(A.detach().to(torch.float16))
                self.layers[i].B[mod][slot, :, :r].copy_(B.detach().to(torch.float16))
            self.scale[slot].fill_(scale)
        self.names[slot], self.targets[slot] = name, tuple(targets)
        if {m for t in self.targets for m in t} != before:
            self.on_launches_changed()
        return slot

    def _zero(self, slot):
        for lay in self.layers:
            for t in list(lay.A.values()) + list(lay.B.values()):
                t[slot].zero_()
        self.scale[slot].zero_()

    def unload(self, name):
        """zero the adapter's slot and free it; rows that still select the slot add exactly nothing to finite outputs"""
        slot = self.index(name)
        if slot < 0:
            raise KeyError("unload_adapter: a name")
        before = {m for t in self.targets for m in t}
        with torch.no_grad():
            self._zero(slot)
        self.names[slot], self.targets[slot] = None, ()
        if {m for t in self.targets for m in t} != before:
            self.on_launches_changed()


# ---- float64 statements of the two launches (tests) ---------------------------------------------------------------------------
def _f64(t):
    return np.asarray(t.detach().cpu().numpy(), dtype=np.float64)


def xin_ref(x, rms_weight=None, rms_eps=0.0, gate=None):
    """the base module's input in float64: x, RMSNorm(x) * w (eps as the fp32 value the launch gets), or x * silu(gate)"""
    x64 = _f64(x)
    if rms_weight is not None:
        r = 1.0 / np.sqrt((x64 * x64).mean(-1, keepdims=True) + float(np.float32(rms_eps)))
        return x64 * r * _f64(rms_weight)
    if gate is not None:
        g = _f64(gate)
        return x64 * (g / (1.0 + np.exp(-g)))
    return x64


def shrink_ref(x, A, row_adapter, rms_weight=None, rms_eps=0.0, gate=None):
    """-> (t, mag, gmag), float64 (rows, R): t = A[a] xin, mag = sum |A_i xin_i|, gmag = sum |A_i xin_i| (|g_i| + 6) (zeros
    without a gate); rows with a negative index: zeros"""
    xin, A64, idx = xin_ref(x, rms_weight, rms_eps, gate), _f64(A), row_adapter.detach().cpu().numpy()
    rows, R = xin.shape[0], A64.shape[1]
    t, mag, gmag = np.zeros((rows, R)), np.zeros((rows, R)), np.zeros((rows, R))
    for i in range(rows):
        if idx[i] >= 0:
            prod = A64[idx[i]] * xin[i][None, :]
            t[i], mag[i] = prod.sum(-1), np.abs(prod).sum(-1)
            if gate is not None:
                gmag[i] = (np.abs(prod) * (np.abs(_f64(gate)[i])[None, :] + 6.0)).sum(-1)
    return t, mag, gmag


def expand_ref(y, B, t, scale, row_adapter, j, r0):
    """-> (y', mag), float64 (rows, out): y' = y + scale[a, j] B[a] t[:, r0 : r0 + R_j] (rows with a negative index: y),
    mag = |y| + |scale| sum |B t|"""
    y64, B64, t64 = _f64(y), _f64(B), _f64(t)[:, r0:r0 + B.shape[2]]
    s64, idx = _f64(scale), row_adapter.detach().cpu().numpy()
    out, mag = y64.copy(), np.abs(y64)
    for i in range(y64.shape[0]):
        if idx[i] >= 0:
            prod = B64[idx[i]] * t64[i][None, :]
            out[i] = y64[i] + s64[idx[i], j] * prod.sum(-1)
            mag[i] = np.abs(y64[i]) + abs(s64[idx[i], j]) * np.abs(prod).sum(-1)
    return out, mag
