"""quip_lib::spec_draft / spec_accept_draft: the step of a speculative greedy decode between two chunk passes of k + 1 rows
(csrc/spec_rows.hip.h) -- accept the guessed tokens the model confirmed, emit them and the model's next token, take the
position back behind them, and draft the next guesses by prompt lookup in the caller's prediction and in the text so far.
One launch, one workgroup, nothing read on the host.  DESIGN 4.18 holds the function.  This module defines the two ops
and the restatement of the function on Python lists (accept_draft_ref / draft_ref: what the tests compare the kernels
against and replay the driver's trace with).  LlamaDecoder.generate_speculative is the driver."""
import math

import torch

from . import capi
from . import register_lib as _R

MAX_K = 15                  # guesses per pass
MAX_G = 8                   # longest match length
MAX_CORPUS = 1 << 20        # capacity of hist + capacity of pred
THREADS = 256               # the workgroup of either launch (kSpecThreads)
STATUS_NONFINITE = 1        # row 0 of a pass had no finite log-sum-exp: nothing was emitted
STATUS_POSITION = 2         # the position does not fit hist: nothing was written

try:
    _R._lib.define("spec_draft(Tensor(a!) rows_tok, Tensor(b!) n_draft, Tensor pos, Tensor hist, Tensor pred, Tensor n_pred, "
                   "Tensor(c!) stats, int gmin, int gmax) -> ()")
    _R._lib.define("spec_accept_draft(Tensor argmax, Tensor lse, Tensor(a!) rows_tok, Tensor(b!) n_draft, Tensor(c!) pos, "
                   "Tensor(d!) hist, Tensor pred, Tensor n_pred, Tensor(e!) out, Tensor(f!) out_len, Tensor(g!) stats, "
                   "int gmin, int gmax) -> ()")
except RuntimeError:
    pass


def _check(op, rows_tok, gmin, gmax, operands):
    """rows_tok (k + 1,) int64 on a CUDA device; operands: (name, tensor, dtype, numel or None = any) on the same device"""
    need = _R._need
    need(rows_tok.is_cuda and rows_tok.dtype == torch.int64 and rows_tok.dim() == 1 and rows_tok.is_contiguous(),
         f"{op}: rows_tok must be contiguous int64 (k + 1,) on a CUDA device")
    k = rows_tok.numel() - 1
    need(1 <= k <= MAX_K, f"{op}: k = rows_tok.numel() - 1 = {k} outside 1 .. {MAX_K}")
    need(0 <= int(gmin) <= int(gmax) <= MAX_G, f"{op}: need 0 <= gmin <= gmax <= {MAX_G}, got ({gmin}, {gmax})")
    for name, t, dt, numel in operands:
        need(t.dtype == dt and t.dim() == 1 and t.is_contiguous() and t.device == rows_tok.device
             and (numel is None or t.numel() == numel),
             f"{op}: {name} must be contiguous {dt} ({'n' if numel is None else numel},) on rows_tok's device")
    return k


def _spec_draft_cuda(rows_tok, n_draft, pos, hist, pred, n_pred, stats, gmin, gmax):
    """rows_tok (k + 1,), pos (1,), hist (>= pos + 1,), pred (cap,), stats (4,) int64; n_draft, n_pred (1,) int32
    (include/quip_mi355.h: quip_spec_draft_i64)"""
    i64, i32 = torch.int64, torch.int32
    k = _check("spec_draft", rows_tok, gmin, gmax,
               (("n_draft", n_draft, i32, 1), ("pos", pos, i64, 1), ("hist", hist, i64, None), ("pred", pred, i64, None),
                ("n_pred", n_pred, i32, 1), ("stats", stats, i64, 4)))
    _R._need(hist.numel() >= 1 and hist.numel() + pred.numel() <= MAX_CORPUS,
             f"spec_draft: hist holds 1 .. and hist + pred at most {MAX_CORPUS} ids")
    with torch.cuda.device(rows_tok.device):
        capi.check(capi.lib().quip_spec_draft_i64(
            rows_tok.data_ptr(), n_draft.data_ptr(), pos.data_ptr(), hist.data_ptr(), hist.numel(),
            pred.data_ptr() if pred.numel() else None, n_pred.data_ptr(), pred.numel(), stats.data_ptr(), k, int(gmin),
            int(gmax), _R._stream(rows_tok)), "quip_spec_draft_i64")


def _spec_accept_draft_cuda(argmax, lse, rows_tok, n_draft, pos, hist, pred, n_pred, out, out_len, stats, gmin, gmax):
    """argmax (k + 1,) int64 and lse (k + 1,) fp32: quip_lib::nll_rows' results for the pass; out (cap_out,), out_len (1,)
    int64; the rest as spec_draft (include/quip_mi355.h: quip_spec_accept_draft_i64)"""
    i64, i32 = torch.int64, torch.int32
    n = rows_tok.numel()
    k = _check("spec_accept_draft", rows_tok, gmin, gmax,
               (("argmax", argmax, i64, n), ("lse", lse, torch.float32, n), ("n_draft", n_draft, i32, 1),
                ("pos", pos, i64, 1), ("hist", hist, i64, None), ("pred", pred, i64, None), ("n_pred", n_pred, i32, 1),
                ("out", out, i64, None), ("out_len", out_len, i64, 1), ("stats", stats, i64, 4)))
    _R._need(hist.numel() >= 1 and hist.numel() + pred.numel() <= MAX_CORPUS and out.numel() < 2 ** 31,
             f"spec_accept_draft: hist holds 1 .. and hist + pred at most {MAX_CORPUS} ids")
    with torch.cuda.device(rows_tok.device):
        capi.check(capi.lib().quip_spec_accept_draft_i64(
            argmax.data_ptr(), lse.data_ptr(), rows_tok.data_ptr(), n_draft.data_ptr(), pos.data_ptr(), hist.data_ptr(),
            hist.numel(), pred.data_ptr() if pred.numel() else None, n_pred.data_ptr(), pred.numel(),
            out.data_ptr() if out.numel() else None, out_len.data_ptr(), out.numel(), stats.data_ptr(), k, int(gmin),
            int(gmax), _R._stream(rows_tok)), "quip_spec_accept_draft_i64")


try:
    _R._lib.impl("spec_draft", _spec_draft_cuda, "CUDA")
    _R._lib.impl("spec_accept_draft", _spec_accept_draft_cuda, "CUDA")
    _R._reg_fake("spec_draft", lambda rows_tok, n_draft, pos, hist, pred, n_pred, stats, gmin, gmax: None)
    _R._reg_fake("spec_accept_draft", lambda argmax, lse, rows_tok, n_draft, pos, hist, pred, n_pred, out, out_len, stats,
                 gmin, gmax: None)
except RuntimeError:
    pass


# ---- the function on lists (CPU) ----------------------------------------------------------------------------------------
def draft_ref(hist, pos, pred, k, gmin, gmax):
    """The guesses behind hist[0 .. pos] (inclusive): corpus C = pred ++ hist[0 .. pos]; for g from gmax down to
    max(gmin, 1), g <= pos + 1, the candidates are the end indices e < len(C) - 1 with C[e - g + 1 .. e] equal to the last
    g tokens of hist[0 .. pos], those g tokens inside one segment and avail(e) >= 1 tokens behind e in e's segment; the
    winner is the maximum of (g, min(avail, k), e) -> C[e + 1 .. e + min(avail, k)] ([] without a candidate)"""
    pred, text = [int(x) for x in pred], [int(x) for x in hist[:pos + 1]]
    C, seam = pred + text, len(pred)
    best = None
    for g in range(int(gmax), max(int(gmin), 1) - 1, -1):
        if g > pos + 1:
            continue
        suffix = text[len(text) - g:]
        for e in range(len(C) - 1):
            first, last = (0, seam) if e < seam else (seam, len(C))      # e's segment [first, last)
            avail = last - 1 - e
            if e - g + 1 < first or avail < 1 or C[e - g + 1:e + 1] != suffix:
                continue
            key = (g, min(avail, k), e)
            if best is None or key > best:
                best = key
    if best is None:
        return []
    _, c, e = best
    return C[e + 1:e + 1 + c]


def accept_draft_ref(state, argmax, lse, k, gmin, gmax):
    """One step of the function on a state dict of Python values -> the new state (the argument is left alone).
    state: rows_tok [k + 1], n_draft, pos (= p0 + k + 1), hist [>= p0 + k + 2], pred [n_pred], out [cap_out], out_len,
    stats [passes, drafted, accepted, status].  argmax / lse: the k + 1 results of nll_rows for the pass.
    argmax=None: the draft alone (spec_draft: pos is p0 and stays, rows_tok[0] stays)."""
    st = {key: (list(v) if isinstance(v, (list, tuple)) else v) for key, v in state.items()}
    n = k + 1
    rows = st["rows_tok"]
    if argmax is None:
        pos, t = st["pos"], rows[0]
    else:
        p0, d = st["pos"] - n, st["n_draft"]
        a = -1
        for j in range(d + 1):
            if not math.isfinite(lse[j]) or (j > 0 and int(argmax[j - 1]) != rows[j]):
                break
            a = j
        if a < 0:
            st["stats"][3] |= STATUS_NONFINITE
            st["pos"] = p0
            return st
        t = int(argmax[a])
        for i, token in enumerate(rows[1:a + 1] + [t]):
            if st["out_len"] + i < len(st["out"]):
                st["out"][st["out_len"] + i] = token
            st["hist"][p0 + 1 + i] = token
        st["out_len"] += a + 1
        pos = st["pos"] = p0 + a + 1
        st["stats"][0] += 1
        st["stats"][1] += d
        st["stats"][2] += a
    guesses = draft_ref(st["hist"], pos, st["pred"], k, gmin, gmax)
    st["n_draft"] = len(guesses)
    st["rows_tok"] = [t] + guesses + [0] * (k - len(guesses))
    return st
