#!/usr/bin/env python3
"""The device sampler (quip_lib::sample_step, csrc/sample_rows.hip.h) against the torch expression it stands beside
(LlamaDecoder.sample), in one process.

The op alone on (1, 32000), (16, 32000) and (31, 128256) fp16 logits (randn * 4), four settings each: temperature only,
top-k 40, top-p 0.9, top-k 40 + top-p 0.9.  The torch expression has no top-p: it is timed with the same temperature and
top-k (None where the setting has none), so the top-p lines compare unequal work and say so.  Both candidates are warmed up
at every shape and setting, then timed ALTERNATING with device events (20 runs of 20 calls each); medians and the spread
(min .. max) are printed.

Not here: a decoder step on this tail (the decoders do not use the op yet)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402
from quip_for_all_amd import sampler as S  # noqa: E402,F401  (defines quip_lib::sample_step)

DEV = "cuda:0"
OP_SHAPES = ((1, 32000), (16, 32000), (31, 128256))
SETTINGS = (("T 0.8", 0.8, 0, 1.0), ("T 0.8 top-k 40", 0.8, 40, 1.0), ("T 0.8 top-p 0.9", 0.8, 0, 0.9),
            ("T 0.8 top-k 40 top-p 0.9", 0.8, 40, 0.9))
ROUNDS = 20            # timed runs per candidate, alternating
REPS = 20              # calls per timed run


def device_ms(fn, reps):
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


def alternate(cands, rounds, reps):
    for fn in cands.values():                   # warm-up of every candidate
        for _ in range(3):
            fn()
    times = {name: [] for name in cands}
    for _ in range(rounds):
        for name, fn in cands.items():
            times[name].append(device_ms(fn, reps))
    return times


@torch.no_grad()
def op_alone():
    for rows, n in OP_SHAPES:
        g = torch.Generator(device=DEV).manual_seed(n + rows)
        logits = (torch.randn(rows, n, generator=g, device=DEV) * 4).half()
        tok = torch.zeros(rows, dtype=torch.int64, device=DEV)
        pos = torch.zeros(rows, dtype=torch.int64, device=DEV)
        seed = torch.arange(rows, dtype=torch.int64, device=DEV)
        for label, T, k, p in SETTINGS:
            tt = torch.full((rows,), T, dtype=torch.float32, device=DEV)
            kk = torch.full((rows,), k, dtype=torch.int32, device=DEV)
            pp = torch.full((rows,), p, dtype=torch.float32, device=DEV)

            def op():
                torch.ops.quip_lib.sample_step(logits, tt, kk, pp, seed, tok, pos)

            def expr():
                tok.copy_(D.LlamaDecoder.sample(logits, T, k or None))
                pos.add_(1)
            times = alternate({"sample_step op": op, "torch expression": expr}, ROUNDS, REPS)
            for name, ts in times.items():
                print(f"op ({rows}, {n}) {label:25s} {name:17s} {fmt(ts)}", flush=True)
            med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
            note = "  [the expression has no top-p: it ran without the cut]" if p < 1.0 else ""
            print(f"op ({rows}, {n}) {label:25s} torch / op = {med['torch expression'] / med['sample_step op']:.2f} (medians){note}",
                  flush=True)


if __name__ == "__main__":
    op_alone()
