"""quip_lib::sample_step: one token per row of (rows, n) fp16 logits, every row with its own temperature, top-k, top-p and
seed, in one launch (csrc/sample_rows.hip.h) -- the sampling tail of a decode step as a deterministic function of (the
row's bits, T, k, p, seed, position).  DESIGN 4.16 holds the function.  This module defines the op and the float64
restatement of the function on the CPU (sample_step_ref: what the tests compare the kernel against, draw by draw).
The decoders do not call it yet."""
import math

import numpy as np
import torch

from . import capi
from . import register_lib as _R

DELTA = 2.0 ** -18          # relative error bound of any prefix mass of the kernel (derived in csrc/sample_rows.hip.h)
MAX_N = 1 << 20             # the longest row the launch takes
_G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1

try:
    _R._lib.define("sample_step(Tensor logits, Tensor temperature, Tensor top_k, Tensor top_p, Tensor seed, "
                   "Tensor(a!) tok, Tensor(b!) pos, Tensor(c!)? kept=None) -> ()")
except RuntimeError:
    pass


def _sample_step_cuda(logits, temperature, top_k, top_p, seed, tok, pos, kept=None):
    """logits (rows, n) fp16 contiguous (any 2-byte aligned start); temperature / top_p (rows,) fp32, top_k (rows,) int32,
    seed / tok / pos (rows,) int64, kept (rows,) int32 or None, all contiguous on the logits' device
    (include/quip_mi355.h: quip_sample_step_f16)"""
    need = _R._need
    need(logits.is_cuda and logits.dtype == torch.float16 and logits.dim() == 2 and logits.is_contiguous(),
         "sample_step: logits must be contiguous float16 (rows, n) on a CUDA device")
    rows, n = logits.shape
    need(rows >= 1 and 1 <= n <= MAX_N, f"sample_step: at least one row, 1 .. {MAX_N} logits")
    for name, t, dt in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32),
                        ("top_p", top_p, torch.float32), ("seed", seed, torch.int64), ("tok", tok, torch.int64),
                        ("pos", pos, torch.int64), ("kept", kept, torch.int32)):
        if t is None and name == "kept":
            continue
        need(t.dtype == dt and tuple(t.shape) == (rows,) and t.is_contiguous() and t.device == logits.device,
             f"sample_step: {name} must be contiguous {dt} (rows,) on the logits' device")
    with torch.cuda.device(logits.device):
        capi.check(capi.lib().quip_sample_step_f16(logits.data_ptr(), rows, n, temperature.data_ptr(), top_k.data_ptr(),
                                                   top_p.data_ptr(), seed.data_ptr(), tok.data_ptr(), pos.data_ptr(),
                                                   None if kept is None else kept.data_ptr(), _R._stream(logits)),
                   "quip_sample_step_f16")


try:
    _R._lib.impl("sample_step", _sample_step_cuda, "CUDA")
    _R._reg_fake("sample_step", lambda logits, temperature, top_k, top_p, seed, tok, pos, kept=None: None)
except RuntimeError:
    pass


# ---- the function in float64 (CPU) ------------------------------------------------------------------------------------
def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def sample_hash(seed, pos):
    """h = mix(mix(seed + G) + G (pos + 1)) mod 2^64 (splitmix64's finaliser; seed / pos: Python ints, any sign)"""
    return _mix((_mix((int(seed) + _G) & _M64) + _G * ((int(pos) + 1) & _M64)) & _M64)


def sample_uniform(seed, pos):
    """u = ((h >> 40) + 0.5) 2^-24, exact in float64"""
    return ((sample_hash(seed, pos) >> 40) + 0.5) * 2.0 ** -24


def sample_dist_ref(x, temperature, top_k, top_p):
    """What a row's draw is made from, everything but the uniform: x (n,) fp16 (numpy or torch), the parameters as the
    kernel reads them (fp32 / int32 / fp32).  -> dict: greedy (bool); token (greedy rows: the arg-max rule's); kept;
    order (kept,) the kept tokens in canonical order; cum (kept,) float64 inclusive cumulative masses in that order
    (token order[i] owns [cum[i - 1], cum[i])); Z = cum[-1]; margin = min_j |mass above class j - p Z_k| / Z_k over the
    classes j >= 2 that top-k kept (inf without top-p)."""
    x = np.asarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float16).reshape(-1)
    n = x.size
    T, k, p = float(np.float32(temperature)), int(top_k), float(np.float32(top_p))
    v = x.astype(np.float64)
    notnan = ~np.isnan(v)
    best = v[notnan].max() if notnan.any() else -np.inf
    if not (T > 0.0) or not np.isfinite(best):
        has = notnan.any() and best > -np.inf
        return {"greedy": True, "token": int(np.flatnonzero(v == best)[0]) if has else 0, "kept": 1, "margin": math.inf}
    idx = np.flatnonzero(np.isfinite(v))
    order = idx[np.argsort(-v[idx], kind="stable")]            # classes descending, inside a class by ascending index
    vs = v[order]
    if 1 <= k < n and k < order.size:
        order = order[vs >= vs[k - 1]]
        vs = v[order]
    w = np.exp((vs - vs[0]) / T)
    cum = np.cumsum(w)
    margin = math.inf
    if 0.0 < p < 1.0:
        zk = cum[-1]
        first = np.flatnonzero(np.diff(vs, prepend=np.inf) != 0)      # where each class starts in `order`
        above = np.where(first > 0, cum[first - 1], 0.0)                # mass strictly above the class
        if first.size > 1:
            margin = float(np.abs(above[1:] - p * zk).min() / zk)
        stays = above < p * zk
        stays[0] = True
        n_cls = int(stays.sum())                                        # (above ascends: the kept classes are a prefix)
        end = first[n_cls] if n_cls < first.size else order.size
        order, cum = order[:end], cum[:end]
    return {"greedy": False, "kept": int(order.size), "order": order, "cum": cum, "Z": float(cum[-1]), "margin": margin}


def sample_draw_ref(dist, seed, pos):
    """the token of a sample_dist_ref() answer at (seed, pos): the first one in canonical order whose cumulative mass
    exceeds u Z"""
    if dist["greedy"]:
        return dist["token"]
    i = int(np.searchsorted(dist["cum"], sample_uniform(seed, pos) * dist["Z"], side="right"))
    return int(dist["order"][min(i, dist["order"].size - 1)])


def sample_accepts(dist, token, seed, pos, delta=DELTA):
    """the draw acceptance rule: `token` passes iff its float64 interval [lo, hi) comes within delta Z of u Z (a greedy
    row: iff it is the arg-max rule's token)"""
    if dist["greedy"]:
        return int(token) == dist["token"]
    at = np.flatnonzero(dist["order"] == int(token))
    if at.size != 1:
        return False
    i, Z = int(at[0]), dist["Z"]
    lo, hi, t = (dist["cum"][i - 1] if i else 0.0), dist["cum"][i], sample_uniform(seed, pos) * Z
    return bool(lo - delta * Z <= t < hi + delta * Z)


def sample_step_ref(logits, temperature, top_k, top_p, seed, pos):
    """The function of quip_lib::sample_step in float64 on the CPU: logits (rows, n) fp16, the other arguments (rows,)
    (tensors, arrays or lists).  -> one dict per row: sample_dist_ref's answer plus token, u, and, for a sampled row,
    lo / hi (kept,): the canonical cumulative intervals [lo[i], hi[i]) of order[i].  Nothing is written: the caller
    advances pos."""
    def col(a):
        return a.detach().cpu().tolist() if isinstance(a, torch.Tensor) else list(np.asarray(a).reshape(-1).tolist())
    x = logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else np.asarray(logits)
    x = x.reshape(-1, x.shape[-1])
    T, K, P, S, C = (col(a) for a in (temperature, top_k, top_p, seed, pos))
    out = []
    for r in range(x.shape[0]):
        d = sample_dist_ref(x[r], T[r], K[r], P[r])
        d["u"] = sample_uniform(S[r], C[r])
        d["token"] = sample_draw_ref(d, S[r], C[r])
        if not d["greedy"]:
            d["hi"] = d["cum"]
            d["lo"] = np.concatenate([[0.0], d["cum"][:-1]])
        out.append(d)
    return out
