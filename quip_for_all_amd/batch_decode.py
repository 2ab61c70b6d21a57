"""Batched decode: up to `QuantLinear.skinny_max_rows` independent sequences in lockstep, each at its own cache position.

`LlamaDecoder.batched(B)` shares the parent's modules, embeddings, norms, lm_head, window and rotary tables and owns B
KV caches, B token / position counters, an attention workspace and its own captured step.  One step of B tokens runs,
per block, the products at M = B rows (whatever `QuantLinear.regime(B)` picks: rows_exact while one rows-mode pass
carries the rows -- bit identical to bs = 1 per row -- and the single-pass skinny kernel beyond) and ONE attention
launch for all sequences (quip_lib::rope_attn_decode_batched: per sequence the arithmetic of the bs = 1 launch);
the greedy tail picks B tokens in one launch (quip_lib::argmax_step_batched).

Slots are independent: `fill_slot(b, prompt)` restarts slot b (its prompt pass writes only slot b's cache) and
`extend_slot(b, tokens)` appends to it while the others keep their state, which is all continuous batching needs from
the decoder.  `fill_slots` / `extend_slots` do the same for SEVERAL slots in one ragged prompt pass: the rows of all
prompts go through every block together and attention is one quip_lib::rope_attn_ragged launch per block
(csrc/ragged_attn.hip.h), so B short prompts cost ceil(sum of lengths / chunk) passes instead of B."""
import math
from functools import partial

import torch
import torch.nn.functional as F

from . import capi
from . import ragged_attn as _ragged_attn
from . import register_lib as _R
from . import score as _score
from .decode import PROJECTIONS, capture_graph
from .qlinear import QuantLinear

try:
    # B sequences: q (B, heads, hd), k / v (B, kv_heads, hd), pos (B,), caches (B, kv_heads, max_len, hd)
    _R._lib.define("rope_attn_decode_batched(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, "
                   "Tensor(a!) kcache, Tensor(b!) vcache, Tensor(c!)? workspace, int window=0) -> Tensor")
    # greedy tail over (B, vocab) logits: tok[b] <- argmax of row b, pos[b] += 1
    _R._lib.define("argmax_step_batched(Tensor logits, Tensor(a!) tok, Tensor(b!) pos) -> ()")
    # rope_attn_decode_batched on sequences that begin at cache row start[b] (left-padded batches): start (B,) int64
    _R._lib.define("rope_attn_decode_batched_start(Tensor q, Tensor k, Tensor v, Tensor cos, Tensor sin, Tensor pos, "
                   "Tensor start, Tensor(a!) kcache, Tensor(b!) vcache, Tensor(c!)? workspace, int window=0) -> Tensor")
except RuntimeError:
    pass


def rope_attn_batched_workspace(batch, heads, head_dim, device):
    """zeroed scratch for the split (long context) mode of rope_attn_decode_batched; allocate once, reuse"""
    return torch.zeros(capi.lib().quip_rope_attn_batched_workspace_bytes(batch, heads, head_dim), dtype=torch.uint8,
                       device=device)


def _decode_batched(entry, q, k, v, cos, sin, pos, kcache, vcache, workspace, window, *more):
    """the checks and the call of the contiguous batched decode launches; more: what an entry takes behind the stream"""
    B, heads, kvh, hd, max_len, _ = _R._check_attn("rope_attn_decode_batched", "batched", q, k, v, cos, sin, pos, kcache, vcache)
    _R._check_attn_workspace(workspace, q, B, heads, hd)
    out = torch.empty_like(q)
    _R._attn_call(entry, q, *_R._ptrs(q, k, v, cos, sin, pos, kcache, vcache, out), B, heads, kvh, hd, max_len,
                  1.0 / math.sqrt(hd), int(window), _R._ptr(workspace), _R._stream(q), *more)
    return out


def _rope_attn_decode_batched_cuda(q, k, v, cos, sin, pos, kcache, vcache, workspace=None, window=0):
    return _decode_batched("quip_rope_attn_decode_batched_f16", q, k, v, cos, sin, pos, kcache, vcache, workspace, window)


def _rope_attn_decode_batched_start_cuda(q, k, v, cos, sin, pos, start, kcache, vcache, workspace=None, window=0):
    """rope_attn_decode_batched for sequences whose tokens are cache rows start[b] .. pos[b] (csrc/decode_glue.hip,
    StartAttnArgs): rotary position of row t is t - start[b], rows below start[b] are never read"""
    _R._need(start.dtype == torch.int64 and tuple(start.shape) == tuple(pos.shape) and start.is_contiguous()
             and start.device == q.device, "start must be a contiguous int64 (B,) tensor on q's device")      # (pos: checked below)
    return _decode_batched("quip_rope_attn_decode_batched_start_f16", q, k, v, cos, sin, pos, kcache, vcache, workspace, window,
                           start.data_ptr())


def _argmax_step_batched_cuda(logits, tok, pos):
    _R._need(logits.dtype == torch.float16 and logits.is_contiguous() and logits.dim() == 2 and logits.is_cuda,
             "argmax_step_batched: logits must be contiguous float16 (B, n)")
    B = logits.shape[0]
    _R._need(all(t.dtype == torch.int64 and tuple(t.shape) == (B,) and t.is_contiguous() and t.device == logits.device
                 for t in (tok, pos)), "tok / pos: contiguous int64 (B,) on the logits' device")
    with torch.cuda.device(logits.device):
        capi.check(capi.lib().quip_argmax_step_batched_f16(logits.data_ptr(), B, logits.shape[1], tok.data_ptr(),
                                                           pos.data_ptr(), _R._stream(logits)),
                   "quip_argmax_step_batched_f16")


try:
    _R._lib.impl("rope_attn_decode_batched", _rope_attn_decode_batched_cuda, "CUDA")
    _R._lib.impl("argmax_step_batched", _argmax_step_batched_cuda, "CUDA")
    _R._reg_fake("rope_attn_decode_batched",
                 lambda q, k, v, cos, sin, pos, kcache, vcache, workspace=None, window=0: torch.empty_like(q))
    _R._reg_fake("argmax_step_batched", lambda logits, tok, pos: None)
    _R._lib.impl("rope_attn_decode_batched_start", _rope_attn_decode_batched_start_cuda, "CUDA")
    _R._reg_fake("rope_attn_decode_batched_start",
                 lambda q, k, v, cos, sin, pos, start, kcache, vcache, workspace=None, window=0: torch.empty_like(q))
except RuntimeError:
    pass


def plan_ragged_passes(lengths, chunk, max_segments=_ragged_attn.MAX_SEGMENTS):
    """Split segments of `lengths[s]` tokens into prompt passes of at most `chunk` rows and `max_segments` segments:
    -> [[(segment, start, rows), ...], ...].  Segments are taken in order; one that does not fit the pass's remaining
    budget is split there and continues in the next pass.  So a segment appears at most once per pass, its pieces are
    consecutive and in order, every token is covered exactly once and no pass is empty.  Pure host arithmetic."""
    chunk, max_segments = int(chunk), int(max_segments)
    if chunk < 1 or max_segments < 1:
        raise ValueError(f"plan_ragged_passes: chunk {chunk}, max_segments {max_segments} (both >= 1)")
    passes, cur, room = [], [], chunk
    for s, n in enumerate(lengths):
        start, n = 0, int(n)
        while start < n:
            if room == 0 or len(cur) == max_segments:
                passes.append(cur)
                cur, room = [], chunk
            rows = min(n - start, room)
            cur.append((s, start, rows))
            start, room = start + rows, room - rows
    if cur:
        passes.append(cur)
    return passes


def _check_ragged(dec, slots, token_lists, what):
    """what extend_slots / fill_slots refuse, before anything is written -> (slots, 1-D id tensors on the device)"""
    slots = [int(b) for b in slots]
    token_lists = list(token_lists)
    if len(slots) != len(token_lists):
        raise ValueError(f"{what}: {len(slots)} slots for {len(token_lists)} token lists (length mismatch)")
    if len(set(slots)) != len(slots):
        raise ValueError(f"{what}: a duplicate slot in {slots} (one launch continues a slot once)")
    for b in slots:
        if not 0 <= b < dec.batch:
            raise ValueError(f"{what}: slot {b} of {dec.batch} is out of range")
    toks = [torch.as_tensor(t, dtype=torch.long, device=dec.dev).reshape(-1) for t in token_lists]
    if any(t.numel() < 1 for t in toks):
        raise ValueError(f"{what}: an empty token list")
    if dec.s.head_dim not in (64, 128):
        raise NotImplementedError(f"head_dim {dec.s.head_dim}: the ragged attention launch serves 64 and 128")
    return slots, toks


def _check_passes(dec, what, slots, token_lists, chunk):
    """the argument checks of extend_slots / score_slots -> (slots, 1-D id tensors on the device)"""
    slots, toks = _check_ragged(dec, slots, token_lists, what)
    if int(chunk) < 1:
        raise ValueError(f"{what}: chunk {int(chunk)} < 1")
    return slots, toks


def _ragged_passes(dec, slots, toks, chunk, on_pass):
    """the pass loop of extend_slots() / score_slots() on checked arguments: per pass of plan_ragged_passes every block
    over the pass's rows and the positions advanced on the device; on_pass(pieces, h) gets the pass's pieces
    [(list, start, rows)] and its hidden rows h (n, hidden)"""
    p, s = dec.parent, dec.s
    for pieces in plan_ragged_passes([t.numel() for t in toks], int(chunk)):
        seg_slot, seg_rows = [slots[j] for j, _, _ in pieces], [r for _, _, r in pieces]
        n = sum(seg_rows)

        def attend(i, q, k, v):
            return dec._attend_ragged(i, q.view(n, s.heads, s.head_dim), k.view(n, s.kv_heads, s.head_dim),
                                      v.view(n, s.kv_heads, s.head_dim), seg_slot, seg_rows).reshape(n, s.q_width)
        h = p.embed[torch.cat([toks[j][a:a + r] for j, a, r in pieces])]      # (n, hidden)
        rows_adapter = None
        if p.lora is not None:
            # every segment's slot adapter over the segment's rows, on the device (nothing read on the host)
            rows_adapter = torch.repeat_interleave(dec.slot_adapter[torch.tensor(seg_slot, dtype=torch.long, device=dec.dev)],
                                                   torch.tensor(seg_rows, dtype=torch.long, device=dec.dev), output_size=n)
        for i, L in enumerate(p.layers):
            h = p._block(L, h, partial(attend, i), adapter=rows_adapter)
        dec.pos.index_add_(0, torch.tensor(seg_slot, dtype=torch.long, device=dec.dev),
                            torch.tensor(seg_rows, dtype=torch.long, device=dec.dev))
        on_pass(pieces, h)


def _no_prompts(dec, what):
    """the prompt-side passes are defined for sequences that begin at cache row 0: a padded decoder refuses them"""
    if getattr(dec, "start", None) is not None:
        raise NotImplementedError(f"{what}: the prompt-side passes write sequences that begin at cache row 0; a "
                                  "padded=True decoder takes its cache rows, pos and start from the caller")


class BatchDecoder:
    """B sequences decoded in lockstep on the modules of a LlamaDecoder (see the module docstring).

    tok / pos: (B,) int64 on the device, the current token and position of every slot.  A slot whose position left
    [0, max_len) gets NaN logits and leaves its cache alone; the other slots are unaffected.

    padded=True: every slot has a first cache row, start (B,) int64 on the device, zeros to begin with -- slot b's tokens
    are cache rows start[b] .. pos[b] and row t has rotary position t - start[b] (a left-padded batch as HF generate
    caches it; quip_lib::rope_attn_decode_batched_start).  The caller writes the cache rows, pos and start; step,
    decode, capture and reset work (a captured step reads start in place), the prompt-side methods, which are defined
    for sequences that begin at row 0, raise NotImplementedError.  A slot with start outside [0, pos] idles like one
    whose position left the cache."""

    def __init__(self, parent, batch, max_len=None, padded=False):
        batch = int(batch)
        if not 1 <= batch <= QuantLinear.skinny_max_rows:
            raise ValueError(f"batch {batch}: 1 .. QuantLinear.skinny_max_rows = {QuantLinear.skinny_max_rows} sequences")
        max_len = parent.max_len if max_len is None else int(max_len)
        if not 1 <= max_len <= parent.max_len:
            raise ValueError(f"max_len {max_len}: 1 .. the parent decoder's max_len = {parent.max_len}")
        if parent.single_copy:
            raise ValueError("a single_copy decoder keeps only the tiled codes of the bs=1 launch: batched decode would "
                             "untile every block at every step")
        s = parent.s
        if s.head_dim not in (64, 128):
            raise NotImplementedError(f"head_dim {s.head_dim}: the batched attention launch serves 64 and 128")
        self.parent, self.batch, self.max_len, self.s, self.dev = parent, batch, max_len, s, parent.dev
        self.window = parent.window
        self.cos, self.sin = parent.cos[:max_len], parent.sin[:max_len]
        self._alloc_cache()
        self.tok = torch.zeros(batch, dtype=torch.long, device=self.dev)
        self.pos = torch.zeros(batch, dtype=torch.long, device=self.dev)
        self.start = torch.zeros(batch, dtype=torch.long, device=self.dev) if padded else None
        self.attn_ws = rope_attn_batched_workspace(batch, s.heads, s.head_dim, self.dev)
        self.graph = None
        self.sampling = None
        self.step_logits = None
        # LoRA (the parent's enable_lora, before or after this decoder was made): one adapter index per slot, -1 = none,
        # read in place by the step; the parent drops this decoder's captured step when the launching groups change
        self.slot_adapter = torch.full((batch,), -1, dtype=torch.int32, device=self.dev)
        parent._lora_dependents.add(self)

    def set_slot_adapter(self, b, name):
        """slot b's adapter from now on (a name of the parent's load_adapter; None: none) -- written on the device, a
        captured step reads it in place.  reset() keeps it."""
        if not 0 <= int(b) < self.batch:
            raise ValueError(f"slot {b} of {self.batch} is out of range")
        self.slot_adapter[int(b):int(b) + 1].fill_(self.parent._need_lora().index(name))

    # the cache and the two attention launches on it: what paged_cache.PagedBatchDecoder replaces
    def _alloc_cache(self):
        s = self.s
        self.kcache = torch.zeros(s.layers, self.batch, s.kv_heads, self.max_len, s.head_dim, dtype=torch.float16,
                                  device=self.dev)
        self.vcache = torch.zeros_like(self.kcache)

    def _fuses_norm(self):
        """does _attend_step normalise q and k itself (a model with q / k norms: LlamaDecoder.qk_norm)?  The contiguous
        launch has an instantiation that does; the padded-start launch -- and the paged ones -- get them normalised by
        LlamaDecoder._block (quip_lib::qk_norm_rows in front: the same bits)"""
        return self.parent.qk_norm and self.parent.qk_fused and self.start is None

    def _attend_step(self, i, q, k, v):
        """block i of step(): q (B, heads, hd), k / v (B, kv_heads, hd) -> (B, heads, hd)"""
        if self._fuses_norm():
            L = self.parent.layers[i]
            return torch.ops.quip_lib.rope_attn_decode_batched_qknorm(q, k, v, self.cos, self.sin, self.pos, self.kcache[i],
                                                                      self.vcache[i], self.attn_ws, self.window,
                                                                      L["q_norm"], L["k_norm"], self.parent.qk_eps)
        if self.start is not None:
            return torch.ops.quip_lib.rope_attn_decode_batched_start(q, k, v, self.cos, self.sin, self.pos, self.start,
                                                                     self.kcache[i], self.vcache[i], self.attn_ws,
                                                                     self.window)
        return torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, self.cos, self.sin, self.pos, self.kcache[i],
                                                           self.vcache[i], self.attn_ws, self.window)

    def _attend_ragged(self, i, q, k, v, seg_slot, seg_rows):
        """block i of a ragged pass: q (rows, heads, hd), k / v (rows, kv_heads, hd) -> (rows, heads, hd)"""
        _no_prompts(self, "a ragged prompt pass")
        return torch.ops.quip_lib.rope_attn_ragged(q, k, v, self.cos, self.sin, self.pos, seg_slot, seg_rows,
                                                   self.kcache[i], self.vcache[i], self.window)

    def regimes(self):
        """the product path of every module of a block at M = B (QuantLinear.regime)"""
        L0 = self.parent.layers[0]
        return {k: L0[k].regime(self.batch) for k in PROJECTIONS}

    def step(self):
        """one token for every slot: reads tok / pos, writes the next tokens into tok, advances pos; returns the
        logits (B, vocab)"""
        p, s, B = self.parent, self.s, self.batch
        h = p.embed[self.tok]                                       # (B, hidden)

        def attend(i, q, k, v):
            return self._attend_step(i, q.view(B, s.heads, s.head_dim), k.view(B, s.kv_heads, s.head_dim),
                                     v.view(B, s.kv_heads, s.head_dim)).reshape(B, s.q_width)
        fused = self._fuses_norm()
        adapter = self.slot_adapter if p.lora is not None else None
        for i, L in enumerate(p.layers):
            h = p._block(L, h, partial(attend, i), norm_in_attend=fused, adapter=adapter)
        return self._head(h)

    def _head(self, h):
        p, s = self.parent, self.s
        logits = F.rms_norm(h, (s.hidden,), p.final_norm, s.rms_eps) @ p.lm_head.T
        if self.sampling is None:
            torch.ops.quip_lib.argmax_step_batched(logits, self.tok, self.pos)
        else:
            self.tok.copy_(p.sample(logits, *self.sampling))
            self.pos.add_(1)
        return logits

    def set_sampling(self, temperature=None, top_k=None):
        """greedy (None / 0) or LlamaDecoder's sampler on every row; part of the captured step"""
        new = None if not temperature else (float(temperature), None if top_k is None else int(top_k))
        if new != self.sampling:
            self.sampling, self.graph = new, None

    def reset(self, first_token=1):
        self.tok.fill_(first_token)
        self.pos.zero_()
        if self.start is not None:
            self.start.zero_()

    def capture(self):
        """warm up and capture one step as a hipGraph (before any prompt is written: the warm-up steps write cache
        rows 0 and 1 of every slot)"""
        self.reset()
        self.graph, self.step_logits = capture_graph(lambda: (self.step(), self.step()), self.step)
        self.reset()

    @torch.no_grad()
    def prefill_slot(self, b, tokens):
        """the parent's batched prompt pass over `tokens`, written into slot b's cache rows 0..P-1; pos[b] = P"""
        _no_prompts(self, "prefill_slot")
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        if not 0 <= b < self.batch or not 1 <= tokens.numel() <= self.max_len:
            raise ValueError(f"slot {b} of {self.batch}, {tokens.numel()} prompt tokens (1 .. {self.max_len})")
        return self.parent.prefill(tokens, kv=(self.kcache[:, b], self.vcache[:, b]), pos=self.pos[b:b + 1],
                                   adapter=self.slot_adapter[b:b + 1])

    @torch.no_grad()
    def extend_slot(self, b, tokens, chunk=512):
        """the parent's extend() on slot b: `tokens` (>= 1 ids) appended behind pos[b] in slot b's cache, pos[b] advanced
        on the device; the other slots keep their state.  Returns the last token's logits (1, vocab)."""
        _no_prompts(self, "extend_slot")
        tokens = torch.as_tensor(tokens, dtype=torch.long, device=self.dev).reshape(-1)
        if not 0 <= b < self.batch or tokens.numel() < 1:
            raise ValueError(f"slot {b} of {self.batch}, {tokens.numel()} tokens to append (>= 1)")
        return self.parent.extend(tokens, chunk=chunk, kv=(self.kcache[:, b], self.vcache[:, b]), pos=self.pos[b:b + 1],
                                  adapter=self.slot_adapter[b:b + 1])

    @torch.no_grad()
    def extend_slots(self, slots, token_lists, chunk=512):
        """extend_slot for several slots in one ragged prompt pass: token_lists[j] (>= 1 ids) is appended behind
        pos[slots[j]] in that slot's cache (distinct slots), the positions advance on the device, slots that are not
        named keep cache, tok and pos bit for bit.  The rows of all lists run through every block together, in passes
        of at most `chunk` rows (plan_ragged_passes); per block and pass the attention is ONE launch
        (quip_lib::rope_attn_ragged: per segment the bits of rope_attn_chunk).  Nothing reads pos on the host.  Tokens
        that do not fit a slot's max_len append nothing and give that slot NaN logits (the launch's range rule, per
        segment).  Returns the last-token logits of every list, (len(slots), vocab), in the order of `slots`."""
        _no_prompts(self, "extend_slots")
        slots, toks = _check_passes(self, "extend_slots", slots, token_lists, chunk)
        return self._extend_passes(slots, toks, chunk)

    def _extend_passes(self, slots, toks, chunk):
        """extend_slots on checked arguments"""
        last = [None] * len(slots)

        def keep(pieces, h):
            row = 0
            for j, a, r in pieces:
                row += r
                if a + r == toks[j].numel():
                    last[j] = h[row - 1]
        _ragged_passes(self, slots, toks, chunk, keep)
        return F.rms_norm(torch.stack(last), (self.s.hidden,), self.parent.final_norm, self.s.rms_eps) @ self.parent.lm_head.T

    @torch.no_grad()
    def score_slots(self, slots, token_lists, targets=None, chunk=512):
        """extend_slots that scores its tokens (LlamaDecoder.score for several slots in the ragged passes): token_lists[j]
        is appended behind pos[slots[j]] exactly as extend_slots appends it -- same passes, same launches, the slots that
        are not named keep cache, tok and pos bit for bit -- and after each pass ALL its rows take the final norm, the
        lm_head product and the scoring tail (quip_lib::nll_rows).  Row i of list j is scored against targets[j][i];
        the default is the list's own next token, the last row not scored (-1 -> exactly 0).  Argument errors are
        extend_slots's, raised before anything is written.  Returns (logprobs, argmaxes): per list one (len_j,) fp32
        and one (len_j,) int64 tensor on the device, in the order of `slots`."""
        _no_prompts(self, "score_slots")
        slots, toks = _check_passes(self, "score_slots", slots, token_lists, chunk)
        return self._score_passes(slots, toks, self._check_targets(toks, targets), chunk)

    def _check_targets(self, toks, targets):
        if targets is None:
            return [_score.shifted_targets(t) for t in toks]
        tgts = [torch.as_tensor(t, dtype=torch.long, device=self.dev).reshape(-1) for t in targets]
        if [t.numel() for t in tgts] != [t.numel() for t in toks]:
            raise ValueError("score_slots: every token list needs a target list of its own length")
        return tgts

    def _score_passes(self, slots, toks, tgts, chunk):
        """score_slots on checked arguments"""
        p, s = self.parent, self.s
        lps = [torch.empty(t.numel(), dtype=torch.float32, device=self.dev) for t in toks]
        ams = [torch.empty(t.numel(), dtype=torch.long, device=self.dev) for t in toks]

        def tail(pieces, h):
            logits = F.rms_norm(h, (s.hidden,), p.final_norm, s.rms_eps) @ p.lm_head.T
            lp, am = _score.score_tail(logits, torch.cat([tgts[j][a:a + r] for j, a, r in pieces]))
            row = 0
            for j, a, r in pieces:
                lps[j][a:a + r] = lp[row:row + r]
                ams[j][a:a + r] = am[row:row + r]
                row += r
        _ragged_passes(self, slots, toks, chunk, tail)
        return lps, ams

    @torch.no_grad()
    def fill_slots(self, slots, prompts):
        """fill_slot for several slots at once: every named slot restarts on its prompt (>= 1 ids) -- pos zeroed on the
        device, all but the last token of every prompt through ONE extend_slots call (one-token prompts contribute no
        segment), the last token becomes tok[slot]; the other slots keep their state"""
        _no_prompts(self, "fill_slots")
        slots, prompts = _check_ragged(self, slots, prompts, "fill_slots")
        if not slots:
            return
        idx = torch.tensor(slots, dtype=torch.long, device=self.dev)
        self.pos.index_fill_(0, idx, 0)
        longer = [j for j, pr in enumerate(prompts) if pr.numel() > 1]
        if longer:
            self._extend_passes([slots[j] for j in longer], [prompts[j][:-1] for j in longer], 512)
        self.tok.index_copy_(0, idx, torch.stack([pr[-1] for pr in prompts]))

    @torch.no_grad()
    def fill_slot(self, b, prompt):
        """restart slot b on `prompt` (>= 1 ids): all but its last token through prefill_slot, the last one becomes
        tok[b]; the other slots keep their state"""
        _no_prompts(self, "fill_slot")
        prompt = torch.as_tensor(prompt, dtype=torch.long, device=self.dev).reshape(-1)
        if prompt.numel() < 1:
            raise ValueError("an empty prompt")
        if prompt.numel() > 1:
            self.prefill_slot(b, prompt[:-1])
        else:
            self.pos[b:b + 1].zero_()
        self.tok[b:b + 1].copy_(prompt[-1:])

    @torch.no_grad()
    def decode(self, n_tokens, use_graph=True):
        """n_tokens steps from the current state -> (B, n_tokens) token ids (device)"""
        if use_graph and self.graph is None:
            raise RuntimeError("no captured step: call capture() before any prompt is written")
        out = torch.empty(self.batch, n_tokens, dtype=torch.long, device=self.dev)
        for t in range(n_tokens):
            if use_graph:
                self.graph.replay()
            else:
                self.step_logits = self.step()
            out[:, t] = self.tok
        return out

    @torch.no_grad()
    def generate(self, prompts, n_tokens, use_graph=True, temperature=None, top_k=None, ragged=False):
        """decode n_tokens for each of the B prompts (1-D ids, ragged lengths >= 1) -> (B, n_tokens) token ids.
        ragged: fill all slots with one fill_slots call (the ragged prompt pass on the chunk-attention route: equivalent
        to the slot-by-slot passes, not bit equal) instead of one fill_slot per prompt"""
        _no_prompts(self, "generate")
        prompts = [torch.as_tensor(pr, dtype=torch.long, device=self.dev).reshape(-1) for pr in prompts]
        if len(prompts) != self.batch:
            raise ValueError(f"{len(prompts)} prompts for {self.batch} slots")
        for pr in prompts:
            if not 1 <= pr.numel() or pr.numel() - 1 + n_tokens > self.max_len:
                raise ValueError(f"a prompt of {pr.numel()} tokens + {n_tokens} new ones does not fit max_len {self.max_len}")
        self.set_sampling(temperature, top_k)
        if use_graph and self.graph is None:
            self.capture()
        self.reset()
        if ragged:
            self.fill_slots(range(self.batch), prompts)
        else:
            for b, pr in enumerate(prompts):
                self.fill_slot(b, pr)
        return self.decode(n_tokens, use_graph)
