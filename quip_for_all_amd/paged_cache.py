"""A paged KV cache for batched decode: one pool of 64-position pages shared by the slots, prefix forking.

`PagePool` is the host side of the block table -- free list, reference counts, a host mirror of the table and the slot
lengths; pure Python, no GPU.  `PagedBatchDecoder` (`LlamaDecoder.batched(B, paged=True, pages=N)`) is BatchDecoder on
such a cache: per layer one K and one V pool (n_pages, kv_heads, 64, hd), one int32 block table (B, max_pages) on the
device shared by all layers, and the two paged attention launches (paged_attn.py) in place of the contiguous ones.
Memory follows the live tokens (a slot holds ceil(length / 64) pages, not max_len rows) and `fork_slot` lets several
slots share the full pages of a common prefix.  Per slot the bits -- logits, tokens, cache rows -- are those of the
contiguous BatchDecoder given the same calls.

The invariant the launches rely on (csrc/paged_attn.hip.h): a page a slot appends to is referenced by that slot only.
PagePool keeps it by construction: only FULL pages are ever shared, and a full page is never appended to.

`kv_dtype="fp8"` (`LlamaDecoder.batched(B, paged=True, kv_dtype="fp8", kv_exp=None)`): the pools are torch.uint8, one OCP
e4m3fn byte per element -- the same pages, table and PagePool in half the bytes.  A stored byte c of layer i means
e4m3fn(c) * 2^e, e = kv_exp[i][0] for K and kv_exp[i][1] for V, integers in [-8, 7], default 0; they travel by value in
the launch arguments and are constant for a decoder.  The launches are the _f8 ops of paged_attn.py; the rows a launch
appends are used by it as stored (the round-trip rule of csrc/paged_attn.hip.h), so chunking, captured replays and
forked slots keep giving identical bits.  Against the fp16 cache the results differ by the rounding of K / V to three
mantissa bits."""
import torch

from .batch_decode import BatchDecoder, _check_passes, _check_ragged
from .decode import capture_graph
from .paged_attn import F8_EXP_MAX, F8_EXP_MIN, PAGE, dequant_f8, gather


class PoolExhausted(RuntimeError):
    """the page pool cannot serve a request; nothing was changed"""


class PagePool:
    """Pages of `slots` sequences of at most `max_pages` pages each out of `n_pages`.

    table[b][j]: the page of positions [64 j, 64 j + 64) of slot b, -1: none.  length[b]: positions slot b holds (or
    has reserved).  ref[p]: how many table entries name page p -- after every call; free pages are named by none."""

    def __init__(self, n_pages, slots, max_pages):
        n_pages, slots, max_pages = int(n_pages), int(slots), int(max_pages)
        if n_pages < 1 or slots < 1 or max_pages < 1:
            raise ValueError(f"PagePool: {n_pages} pages, {slots} slots, {max_pages} pages per slot (all >= 1)")
        self.n_pages, self.slots, self.max_pages = n_pages, slots, max_pages
        self.free = list(range(n_pages - 1, -1, -1))        # a stack: page 0 goes out first
        self.ref = [0] * n_pages
        self.table = [[-1] * max_pages for _ in range(slots)]
        self.length = [0] * slots

    def free_count(self):
        return len(self.free)

    def pages_of(self, length):
        return (int(length) + PAGE - 1) // PAGE

    def snapshot(self):
        return list(self.free), list(self.ref), [list(r) for r in self.table], list(self.length)

    def restore(self, snap):
        self.free, self.ref, self.table, self.length = list(snap[0]), list(snap[1]), [list(r) for r in snap[2]], list(snap[3])

    def _slot(self, slot):
        slot = int(slot)
        if not 0 <= slot < self.slots:
            raise ValueError(f"PagePool: slot {slot} of {self.slots}")
        return slot

    def reserve(self, slot, length):
        """pages for positions [0, length) of `slot` (a slot never shrinks here); raises PoolExhausted, before changing
        anything, when the free list is too short.  -> True when the slot's table row changed"""
        slot, length = self._slot(slot), int(length)
        if not 0 <= length <= self.max_pages * PAGE:
            raise ValueError(f"PagePool.reserve: length {length} outside 0 .. {self.max_pages * PAGE}")
        have, want = self.pages_of(self.length[slot]), self.pages_of(length)
        if want - have > len(self.free):
            raise PoolExhausted(f"slot {slot} needs {want - have} more pages for {length} positions, {len(self.free)} are free")
        row = self.table[slot]
        for j in range(have, want):
            p = self.free.pop()
            self.ref[p] = 1
            row[j] = p
        self.length[slot] = max(self.length[slot], length)
        return want > have

    def release(self, slot):
        """drop the slot's references; pages nobody names any more go back to the free list"""
        slot = self._slot(slot)
        row = self.table[slot]
        for j, p in enumerate(row):
            if p < 0:
                continue
            self.ref[p] -= 1
            if self.ref[p] == 0:
                self.free.append(p)
            row[j] = -1
        self.length[slot] = 0

    def fork(self, src, dst):
        """`dst`, released first, continues `src`: it references every FULL page of src and gets a fresh page for src's
        partial last page, if there is one.  -> [(src_page, dst_page)], the pages to copy (none or one).  Raises
        PoolExhausted, before changing anything, when that fresh page cannot be had."""
        src, dst = self._slot(src), self._slot(dst)
        if src == dst:
            raise ValueError(f"PagePool.fork: slot {src} onto itself")
        n = self.length[src]
        full, partial = n // PAGE, n % PAGE != 0
        if partial and not self.free and not any(p >= 0 and self.ref[p] == 1 for p in self.table[dst]):
            raise PoolExhausted(f"fork {src} -> {dst}: no page for the copy of the partial last page")
        self.release(dst)
        srow, drow = self.table[src], self.table[dst]
        for j in range(full):
            drow[j] = srow[j]
            self.ref[srow[j]] += 1
        pairs = []
        if partial:
            p = self.free.pop()
            self.ref[p] = 1
            drow[full] = p
            pairs.append((srow[full], p))
        self.length[dst] = n
        return pairs

    def writable(self, slot):
        """the invariant of the paged launches for `slot`: the page it appends to next is its own"""
        slot = self._slot(slot)
        j = self.length[slot] // PAGE
        if j < self.max_pages and self.table[slot][j] >= 0:
            p = self.table[slot][j]
            assert self.ref[p] == 1, f"slot {slot} would append to page {p}, which {self.ref[p]} table entries name"
        return True

    def check(self):
        """every invariant of the class docstring (tests, debugging)"""
        count = [0] * self.n_pages
        for b, row in enumerate(self.table):
            held = self.pages_of(self.length[b])
            assert all(p >= 0 for p in row[:held]) and all(p == -1 for p in row[held:]), (b, row, self.length[b])
            for p in row[:held]:
                count[p] += 1
        assert count == self.ref, (count, self.ref)
        assert sorted(self.free) == [p for p in range(self.n_pages) if count[p] == 0], self.free
        for b in range(self.slots):
            self.writable(b)
        return True


class PagedBatchDecoder(BatchDecoder):
    """BatchDecoder on a paged cache (see the module docstring).  Members: kpool / vpool (layers, n_pages, kv_heads, 64,
    hd) -- page p is index p in every layer --, table (B, max_pages) int32 on the device, pool (the PagePool: host mirror
    of the table and of the slot lengths).  Pages are assigned on the host before the launches that need them; pos is
    still never read from the device.

    Every slot is live until free_slot() idles it (NaN logits, no cache writes, the launches' range rule); filling,
    extending or forking onto it revives it.  The SDPA prompt route writes contiguous views and does not exist here:
    fill_slot / extend_slot / prefill_slot go through the ragged pass."""

    def __init__(self, parent, batch, max_len=None, pages=None, kv_dtype=None, kv_exp=None):
        if kv_dtype not in (None, "fp16", "fp8"):
            raise ValueError(f"kv_dtype {kv_dtype!r}: None, 'fp16' or 'fp8'")
        self.fp8 = kv_dtype == "fp8"
        if kv_exp is not None and not self.fp8:
            raise ValueError("kv_exp: only with kv_dtype='fp8'")
        self.kv_exp = self._check_kv_exp(kv_exp, parent.s.layers) if self.fp8 else None
        self._pages_arg = pages
        super().__init__(parent, batch, max_len)

    @staticmethod
    def _check_kv_exp(kv_exp, layers):
        """None (all 0), or (layers, 2) ints in [-8, 7] as nested lists or a tensor -> [[k_exp, v_exp]] per layer"""
        if kv_exp is None:
            return [[0, 0] for _ in range(layers)]
        if isinstance(kv_exp, torch.Tensor):
            if kv_exp.is_floating_point() or kv_exp.dtype == torch.bool:
                raise ValueError("kv_exp: an integer tensor")
            kv_exp = kv_exp.tolist()
        try:
            rows = [list(r) for r in kv_exp]
        except TypeError:
            raise ValueError(f"kv_exp: a ({layers}, 2) list or tensor of ints") from None
        if len(rows) != layers or any(len(r) != 2 for r in rows):
            raise ValueError(f"kv_exp: a ({layers}, 2) list or tensor of ints")
        for r in rows:
            for e in r:
                if isinstance(e, bool) or not isinstance(e, int) or not F8_EXP_MIN <= e <= F8_EXP_MAX:
                    raise ValueError(f"kv_exp: ints in [{F8_EXP_MIN}, {F8_EXP_MAX}], got {e!r}")
        return rows

    def _alloc_cache(self):
        s = self.s
        self.max_pages = (self.max_len + PAGE - 1) // PAGE
        n = self.batch * self.max_pages if self._pages_arg is None else int(self._pages_arg)
        if n < 1:
            raise ValueError(f"pages {n}: at least one")
        self.n_pages = n
        self.kpool = torch.zeros(s.layers, n, s.kv_heads, PAGE, s.head_dim,
                                 dtype=torch.uint8 if self.fp8 else torch.float16, device=self.dev)
        self.vpool = torch.zeros_like(self.kpool)
        self.table = torch.full((self.batch, self.max_pages), -1, dtype=torch.int32, device=self.dev)
        self.pool = PagePool(n, self.batch, self.max_pages)
        self.live = [True] * self.batch

    def _fuses_norm(self):
        return False                 # (the paged launches have no q / k norm: LlamaDecoder._block normalises in front)

    def _attend_step(self, i, q, k, v):
        if self.fp8:
            return torch.ops.quip_lib.rope_attn_decode_paged_f8(q, k, v, self.cos, self.sin, self.pos, self.table,
                                                                self.kpool[i], self.vpool[i], self.attn_ws, self.window,
                                                                self.kv_exp[i][0], self.kv_exp[i][1])
        return torch.ops.quip_lib.rope_attn_decode_paged(q, k, v, self.cos, self.sin, self.pos, self.table, self.kpool[i],
                                                         self.vpool[i], self.attn_ws, self.window)

    def _attend_ragged(self, i, q, k, v, seg_slot, seg_rows):
        if self.fp8:
            return torch.ops.quip_lib.rope_attn_ragged_paged_f8(q, k, v, self.cos, self.sin, self.pos, seg_slot, seg_rows,
                                                                self.table, self.kpool[i], self.vpool[i], self.window,
                                                                self.kv_exp[i][0], self.kv_exp[i][1])
        return torch.ops.quip_lib.rope_attn_ragged_paged(q, k, v, self.cos, self.sin, self.pos, seg_slot, seg_rows,
                                                         self.table, self.kpool[i], self.vpool[i], self.window)

    # ---- host side: pages and the device table
    def pages_free(self):
        return self.pool.free_count()

    @property
    def lengths(self):
        """the host mirror of the slot lengths"""
        return list(self.pool.length)

    def _push_table(self):
        """the host table to the device tensor, in place (a captured step reads that tensor)"""
        self.table.copy_(torch.tensor(self.pool.table, dtype=torch.int32))

    def _assign(self, new_lengths, restart=()):
        """all or nothing: release the `restart` slots, reserve pages for new_lengths {slot: length} (beyond max_len the
        launches refuse the rows anyway: reserved up to it), push the table; PoolExhausted leaves everything as it was"""
        snap = self.pool.snapshot()
        try:
            for b in restart:
                self.pool.release(b)
            for b, n in new_lengths.items():
                self.pool.reserve(b, min(int(n), self.max_len))
                self.pool.writable(b)
        except PoolExhausted:
            self.pool.restore(snap)
            raise
        for b in list(restart) + list(new_lengths):
            self.live[b] = True
        self._push_table()

    def gather_slot(self, b):
        """slot b's cache rows [0, length) as contiguous copies -> (K, V), each (layers, kv_heads, length, hd) fp16 (an
        fp8 cache: the values its bytes mean, exact)"""
        k, v = self.gather_slot_raw(b)
        if not self.fp8:
            return k, v
        return tuple(torch.stack([dequant_f8(x[i], self.kv_exp[i][j]) for i in range(self.s.layers)])
                     if x.numel() else x.to(torch.float16) for j, x in enumerate((k, v)))

    def gather_slot_raw(self, b):
        """gather_slot in the pools' own dtype: fp16 rows, or the stored e4m3fn bytes (uint8) of an fp8 cache"""
        n = self.pool.length[b]
        row = torch.tensor(self.pool.table[b][:self.pool.pages_of(n)], dtype=torch.int32, device=self.dev).view(1, -1)
        if n == 0:
            e = self.kpool.new_empty(self.s.layers, self.s.kv_heads, 0, self.s.head_dim)
            return e, e.clone()
        return tuple(torch.stack([gather(pool[i], row)[0, :, :n] for i in range(self.s.layers)])
                     for pool in (self.kpool, self.vpool))

    @torch.no_grad()
    def suggest_kv_exp(self, slots, token_lists):
        """exponents for `kv_exp` from sample prompts: the prompts are cached by a scratch fp16 paged decoder of this
        one's parent, batch and max_len (prompt j in slot slots[j]; this decoder is not touched); per layer and K | V the
        smallest e with absmax * 2^-e <= 448, clipped to [-8, 7] -> [[k_exp, v_exp]] per layer"""
        import math
        slots, toks = _check_ragged(self, slots, token_lists, "suggest_kv_exp")
        if not slots:
            raise ValueError("suggest_kv_exp: at least one prompt")
        scratch = PagedBatchDecoder(self.parent, self.batch, self.max_len,
                                    pages=sum(self.pool.pages_of(t.numel()) for t in toks))
        scratch._assign({b: t.numel() for b, t in zip(slots, toks)})
        scratch._extend_passes(slots, toks, 512)
        out = []
        for i in range(self.s.layers):
            row = []
            for pool in (scratch.kpool, scratch.vpool):
                amax = float(pool[i].float().abs().max())          # (unused pages are zero)
                if not math.isfinite(amax):
                    raise ValueError(f"suggest_kv_exp: layer {i} cached a non-finite value")
                e = math.ceil(math.log2(amax / 448.0)) if amax > 0 else F8_EXP_MIN
                while amax * 2.0 ** -e > 448.0:                     # (log2's rounding)
                    e += 1
                while e > F8_EXP_MIN and amax * 2.0 ** -(e - 1) <= 448.0:
                    e -= 1
                row.append(min(max(e, F8_EXP_MIN), F8_EXP_MAX))
            out.append(row)
        return out

    # ---- slots
    def reset(self, first_token=1):
        """every slot live, empty and at position 0; all pages free"""
        super().reset(first_token)
        for b in range(self.batch):
            self.pool.release(b)
        self.live = [True] * self.batch
        self._push_table()

    def free_slot(self, b):
        """release slot b's pages; the slot idles (NaN logits, no writes) until it is filled, extended or forked onto"""
        self.pool.release(b)
        self.live[int(b)] = False
        self.slot_adapter[int(b):int(b) + 1].fill_(-1)
        self._push_table()

    @torch.no_grad()
    def fork_slot(self, src, dst):
        """slot dst becomes a copy of slot src that shares its full pages: only src's partial last page is copied (in
        every layer); tok and pos of src are copied on the device"""
        pairs = self.pool.fork(src, dst)
        self.live[int(dst)] = self.live[int(src)]
        self._push_table()
        for sp, dp in pairs:
            self.kpool[:, dp].copy_(self.kpool[:, sp])
            self.vpool[:, dp].copy_(self.vpool[:, sp])
        self.tok[dst:dst + 1].copy_(self.tok[src:src + 1])
        self.pos[dst:dst + 1].copy_(self.pos[src:src + 1])
        self.slot_adapter[dst:dst + 1].copy_(self.slot_adapter[src:src + 1])

    def capture(self):
        """BatchDecoder.capture(); the warm-up steps write rows 0 and 1 of every slot, into one page per slot borrowed
        for the purpose and returned.  Raises PoolExhausted if fewer than B pages are free after the reset."""
        self.reset()
        if self.pool.free_count() < self.batch:
            raise PoolExhausted(f"capture() borrows one page per slot: {self.batch} slots, {self.pool.free_count()} pages")
        self._assign({b: PAGE for b in range(self.batch)})
        self.graph, self.step_logits = capture_graph(lambda: (self.step(), self.step()), self.step)
        self.reset()                 # (returns the pages)

    @torch.no_grad()
    def extend_slots(self, slots, token_lists, chunk=512):
        """BatchDecoder.extend_slots; the pages the new rows need are reserved first -- PoolExhausted, with nothing
        written, when the pool is short"""
        slots, toks = _check_passes(self, "extend_slots", slots, token_lists, chunk)
        self._assign({b: self.pool.length[b] + t.numel() for b, t in zip(slots, toks)})
        return self._extend_passes(slots, toks, chunk)

    @torch.no_grad()
    def score_slots(self, slots, token_lists, targets=None, chunk=512):
        """BatchDecoder.score_slots; pages reserved first as in extend_slots"""
        slots, toks = _check_passes(self, "score_slots", slots, token_lists, chunk)
        tgts = self._check_targets(toks, targets)
        self._assign({b: self.pool.length[b] + t.numel() for b, t in zip(slots, toks)})
        return self._score_passes(slots, toks, tgts, chunk)

    @torch.no_grad()
    def fill_slots(self, slots, prompts):
        """BatchDecoder.fill_slots; the named slots give their pages back and get those of their prompts, all or nothing"""
        slots, prompts = _check_ragged(self, slots, prompts, "fill_slots")
        if not slots:
            return
        self._assign({b: pr.numel() - 1 for b, pr in zip(slots, prompts)}, restart=slots)
        idx = torch.tensor(slots, dtype=torch.long, device=self.dev)
        self.pos.index_fill_(0, idx, 0)
        longer = [j for j, pr in enumerate(prompts) if pr.numel() > 1]
        if longer:
            self._extend_passes([slots[j] for j in longer], [prompts[j][:-1] for j in longer], 512)
        self.tok.index_copy_(0, idx, torch.stack([pr[-1] for pr in prompts]))

    def fill_slot(self, b, prompt):
        """fill_slots for one slot (the ragged pass: there is no SDPA prompt route on a paged cache)"""
        self.fill_slots([b], [prompt])

    @torch.no_grad()
    def prefill_slot(self, b, tokens):
        """slot b restarted on `tokens`, all of them cached through the ragged pass; pos[b] = their count.  Returns the
        last token's logits (1, vocab)."""
        slots, toks = _check_ragged(self, [b], [tokens], "prefill_slot")
        self._assign({slots[0]: toks[0].numel()}, restart=slots)
        self.pos[slots[0]:slots[0] + 1].zero_()
        return self._extend_passes(slots, toks, 512)

    def extend_slot(self, b, tokens, chunk=512):
        """extend_slots for one slot -> the last token's logits (1, vocab)"""
        return self.extend_slots([b], [tokens], chunk)

    @torch.no_grad()
    def decode(self, n_tokens, use_graph=True):
        """BatchDecoder.decode; the pages of n_tokens more positions of every live slot are reserved before the first
        step (PoolExhausted otherwise, nothing decoded), so the replays of the captured step need no host work"""
        if use_graph and self.graph is None:
            raise RuntimeError("no captured step: call capture() before any prompt is written")
        self._assign({b: self.pool.length[b] + int(n_tokens) for b in range(self.batch) if self.live[b]})
        return super().decode(n_tokens, use_graph)

    def generate(self, prompts, n_tokens, use_graph=True, temperature=None, top_k=None, ragged=True):
        """BatchDecoder.generate; the prompts always go through fill_slots here"""
        return super().generate(prompts, n_tokens, use_graph, temperature, top_k, ragged=True)
