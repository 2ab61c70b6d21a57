"""quip_lib::nll_rows: log-sum-exp, target log-probability and arg-max of every row of (rows, n) fp16 logits, one launch
and no fp32 copy of the logits (csrc/nll_rows.hip.h) -- the tail of a prompt pass that SCORES its tokens instead of
keeping only the last row.  LlamaDecoder.score / perplexity and BatchDecoder.score_slots build on it; the window plan of
the usual perplexity protocol (plan_score_windows) is host arithmetic and lives here too."""
import os

import torch

from . import capi
from . import register_lib as _R

_NLL_ROWS = os.environ.get("QUIP_NLL_ROWS", "1") != "0"     # A/B switch: 0 = the plain torch tail of score_tail

try:
    _R._lib.define("nll_rows(Tensor logits, Tensor target) -> (Tensor, Tensor, Tensor)")
except RuntimeError:
    pass


def _nll_rows_cuda(logits, target):
    """logits (rows, n) fp16 contiguous, target (rows,) int64 on the same device -> logprob (rows,) fp32, lse (rows,) fp32,
    argmax (rows,) int64.  target < 0: logprob exactly 0 (not scored); target >= n: NaN; a row whose lse is not finite:
    NaN (include/quip_mi355.h: quip_nll_rows_f16)"""
    need = _R._need
    need(logits.is_cuda and logits.dtype == torch.float16 and logits.dim() == 2 and logits.is_contiguous(),
         "nll_rows: logits must be contiguous float16 (rows, n) on a CUDA device")
    rows, n = logits.shape
    need(rows >= 1 and n >= 1, "nll_rows: at least one row and one logit")
    need(target.dtype == torch.int64 and tuple(target.shape) == (rows,) and target.is_contiguous()
         and target.device == logits.device, "nll_rows: target must be contiguous int64 (rows,) on the logits' device")
    logprob = _R._empty(rows, dtype=torch.float32, device=logits.device)
    lse = _R._empty(rows, dtype=torch.float32, device=logits.device)
    argmax = _R._empty(rows, dtype=torch.int64, device=logits.device)
    with torch.cuda.device(logits.device):
        capi.check(capi.lib().quip_nll_rows_f16(logits.data_ptr(), rows, n, target.data_ptr(), logprob.data_ptr(),
                                                lse.data_ptr(), argmax.data_ptr(), _R._stream(logits)), "quip_nll_rows_f16")
    return logprob, lse, argmax


def _nll_rows_fake(logits, target):
    rows = logits.shape[0]
    return (logits.new_empty((rows,), dtype=torch.float32), logits.new_empty((rows,), dtype=torch.float32),
            logits.new_empty((rows,), dtype=torch.int64))


try:
    _R._lib.impl("nll_rows", _nll_rows_cuda, "CUDA")
    _R._reg_fake("nll_rows", _nll_rows_fake)
except RuntimeError:
    pass


def nll_rows_torch(logits, target):
    """the rules of quip_lib::nll_rows as a torch expression on an fp32 copy of the logits -> (logprob, lse, argmax).  What
    QUIP_NLL_ROWS=0 runs, and what tools/score_bench.py times the kernel against.  (argmax of a row with a NaN is torch's:
    the NaN's index.)"""
    x = logits.float()
    n = x.shape[-1]
    lse = torch.logsumexp(x, -1)
    lp = x.gather(-1, target.clamp(0, n - 1)[:, None])[:, 0] - lse
    nan = torch.full_like(lp, float("nan"))
    lp = torch.where(torch.isfinite(lse) & (target < n), lp, nan)
    return torch.where(target < 0, torch.zeros_like(lp), lp), lse, x.argmax(-1)


def score_tail(logits, target):
    """(logprob, argmax) of the rows of a chunk's logits against `target`: the kernel, or -- QUIP_NLL_ROWS=0, for A/B
    runs -- the torch expression"""
    lp, _, am = torch.ops.quip_lib.nll_rows(logits, target) if _NLL_ROWS else nll_rows_torch(logits, target)
    return lp, am


def shifted_targets(tokens):
    """the default targets of a scored token list: row i is scored against token i + 1, the last row is not scored (-1)"""
    return torch.cat([tokens[1:], tokens.new_full((1,), -1)])


def plan_score_windows(n_tokens, window, stride=None, max_len=None):
    """The windows of the usual perplexity protocol over tokens 0 .. n_tokens - 1 -> [(start, length, first_scored)].
    Window w feeds the `length` tokens [start, start + length) from position 0, start = w * stride and
    length = min(window, n_tokens - 1 - start); its row i is scored against token start + i + 1 (so a window reads one
    token past its rows, as a target only).  Rows first_scored .. length - 1 count: all rows of the first window, and
    from the second window on the rows whose target no earlier window scored -- the last `stride` ones of a full window;
    the rows before them are context.  The plan ends with the window whose last target is the last token.  So every
    target position 1 .. n_tokens - 1 is scored exactly once and no window is without a scored row.  stride defaults
    to window (windows that do not overlap); max_len, where given, is the longest window the decoder can hold.  Pure
    host arithmetic."""
    n_tokens, window = int(n_tokens), int(window)
    stride = window if stride is None else int(stride)
    if n_tokens < 2:
        raise ValueError(f"plan_score_windows: {n_tokens} tokens hold no target")
    if window < 2:
        raise ValueError(f"plan_score_windows: window {window} < 2")
    if stride < 1 or stride > window:
        raise ValueError(f"plan_score_windows: stride {stride} outside 1 .. window = {window} (targets would be skipped)")
    if max_len is not None and window > int(max_len):
        raise ValueError(f"plan_score_windows: window {window} > max_len {int(max_len)}")
    plan, done = [], 0                  # done: the first row (its target is token done + 1) that is not scored yet
    for start in range(0, n_tokens - 1, stride):
        length = min(window, n_tokens - 1 - start)
        plan.append((start, length, done - start))
        done = start + length
        if done == n_tokens - 1:
            break
    return plan
