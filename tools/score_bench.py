#!/usr/bin/env python3
"""The scoring tail (quip_lib::nll_rows, csrc/nll_rows.hip.h) against the torch expression it replaces, in one process.

(a) The tail alone on (512, 32000) and (512, 128256) fp16 logits: the kernel against logsumexp + gather on .float() plus
    argmax (score.nll_rows_torch).  Both warmed up at every shape, then timed ALTERNATING with device events (20 runs of 10
    calls each), medians and the spread (min .. max) of every candidate printed.  The kernel reads the fp16 logits once
    (twice past 65536 logits of a row); the torch expression writes and re-reads an fp32 copy.
(b) LlamaDecoder.score of a 2048-token window on the 7B shape (E8P12, chunk 512) with the kernel tail and with the torch
    tail (the module's QUIP_NLL_ROWS flag set by hand between runs): tokens/s (wall clock behind a device synchronise) and
    the peak of torch.cuda.max_memory_allocated above what the decoder itself holds.

  --shape NAME   a shape of quip_for_all_amd.decode instead of LLAMA2_7B for (b) (TINY: a quick run of the tool itself)
  --window N     tokens of (b)'s window (default 2048)
  --skip-model   (a) only"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402
from quip_for_all_amd import score as S  # noqa: E402

DEV = "cuda:0"
TAIL_SHAPES = ((512, 32000), (512, 128256))
TAIL_ROUNDS = 20       # timed runs per candidate, alternating
TAIL_REPS = 10         # calls per timed run
MODEL_ROUNDS = 3


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def device_ms(fn, reps=TAIL_REPS):
    """device-event time of one call, over `reps` back-to-back calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def fmt(ts):
    ts = sorted(ts)
    return f"median {ts[len(ts) // 2] * 1e3:9.1f} us  (min {ts[0] * 1e3:.1f} .. max {ts[-1] * 1e3:.1f}, {len(ts)} runs)"


@torch.no_grad()
def tail_alone():
    for rows, n in TAIL_SHAPES:
        g = torch.Generator(device=DEV).manual_seed(n)
        logits = (torch.randn(rows, n, generator=g, device=DEV) * 4).half()
        target = torch.randint(0, n, (rows,), generator=g, device=DEV)
        cands = {"nll_rows kernel": lambda: torch.ops.quip_lib.nll_rows(logits, target),
                 "torch expression": lambda: S.nll_rows_torch(logits, target)}
        k, t = cands["nll_rows kernel"](), cands["torch expression"]()
        err = float((k[0].double() - t[0].double()).abs().max())
        assert err <= 1e-3 and torch.equal(k[2], t[2]), f"({rows}, {n}): the candidates disagree ({err})"
        for fn in cands.values():               # warm-up of both at this shape
            for _ in range(3):
                fn()
        times = {name: [] for name in cands}
        for _ in range(TAIL_ROUNDS):
            for name, fn in cands.items():
                times[name].append(device_ms(fn))
        for name in cands:
            print(f"tail ({rows}, {n}): {name:17s} {fmt(times[name])}", flush=True)
        med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
        print(f"tail ({rows}, {n}): torch / kernel = {med['torch expression'] / med['nll_rows kernel']:.2f} (medians); "
              f"fp16 logits {rows * n * 2 / 1e6:.1f} MB -> {rows * n * 2 / med['nll_rows kernel'] / 1e6:.0f} GB/s of one read",
              flush=True)


@torch.no_grad()
def window_score():
    name, window = _arg("--shape", "LLAMA2_7B"), int(_arg("--window", "2048"))
    shape = getattr(D, name)
    dec = D.LlamaDecoder(shape, "E8P12", max_len=window, device=DEV, device_init=True)
    toks = torch.randint(0, shape.vocab, (window,), generator=torch.Generator().manual_seed(5)).to(DEV)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated()
    print(f"score(): {name} E8P12, {shape.layers} layers, window {window}, chunk 512; the decoder holds {held / 2**20:.0f} MiB",
          flush=True)

    def run(flag):
        S._NLL_ROWS = flag
        dec.pos.zero_()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        t0 = time.perf_counter()
        lp, _ = dec.score(toks, chunk=512)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, torch.cuda.max_memory_allocated() - held, lp
    res = {True: [], False: []}
    lps = {}
    for flag in (True, False):                  # warm-up of both
        lps[flag] = run(flag)[2]
    err = float((lps[True].double() - lps[False].double()).abs().max())
    print(f"score(): the two tails agree, max logprob difference {err:.2e}", flush=True)
    for _ in range(MODEL_ROUNDS):
        for flag in (True, False):
            res[flag].append(run(flag)[:2])
    for flag, label in ((True, "kernel tail"), (False, "torch tail (QUIP_NLL_ROWS=0)")):
        secs = sorted(s for s, _ in res[flag])
        print(f"score(): {label:29s} median {window / secs[len(secs) // 2]:8.0f} tokens/s  (runs "
              + " ".join(f"{s * 1e3:.1f}" for s, _ in res[flag]) + f" ms)  peak above the decoder {max(m for _, m in res[flag]) / 2**20:.0f} MiB",
              flush=True)
    S._NLL_ROWS = True


if __name__ == "__main__":
    tail_alone()
    if "--skip-model" not in sys.argv:
        window_score()
