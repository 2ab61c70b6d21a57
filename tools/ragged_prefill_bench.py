#!/usr/bin/env python3
"""Filling the slots of a BatchDecoder on the 32-layer 7B decoder (E8P12): one fill_slot per prompt (B whole prompt passes of
the parent decoder, ~600 eager launches each) against ONE fill_slots call (the ragged prompt pass: ceil(sum of lengths /
512) passes, one quip_lib::rope_attn_ragged launch per block and pass).

B = 16, then 4 and 31; ragged prompt lengths in [24, 200] from a fixed seed.  Per B: the first decode step behind both
fills is compared first (0.03 (max|ref| + 1), the tolerance of the prompt-pass tests), then, after one warm-up round of
both, the two are timed ALTERNATING in the same process, five rounds, every run printed: wall time (host clock around
the call and a device synchronise: what a serving loop waits for) and device-event time.

  --shape NAME     a shape of quip_for_all_amd.decode instead of LLAMA2_7B (TINY: a quick run of the tool itself)
  --batches 16,4   the batch sizes, in this order"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402
from quip_for_all_amd.batch_decode import plan_ragged_passes  # noqa: E402

DEV = "cuda:0"
MAX_LEN = 256
LOW, HIGH = 24, 200
ROUNDS = 5


def _arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def timed(fn):
    """(wall ms, device-event ms) of fn(), the wall clock stopped behind a device synchronise"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def fmt(ts):
    return f"best {min(ts):8.2f} ms  median {sorted(ts)[len(ts) // 2]:8.2f}  (runs " + " ".join(f"{t:.2f}" for t in ts) + ")"


@torch.no_grad()
def main():
    shape = getattr(D, _arg("--shape", "LLAMA2_7B"))
    batches = [int(x) for x in _arg("--batches", "16,4,31").split(",")]
    dec = D.LlamaDecoder(shape, "E8P12", max_len=MAX_LEN, device=DEV, device_init=True)
    print(f"{_arg('--shape', 'LLAMA2_7B')} E8P12, {shape.layers} layers, max_len {MAX_LEN}, prompt lengths in [{LOW}, {HIGH}], "
          f"{ROUNDS} alternating rounds after one warm-up round", flush=True)
    for B in batches:
        g = torch.Generator().manual_seed(1000 + B)
        lengths = torch.randint(LOW, HIGH + 1, (B,), generator=g).tolist()
        prompts = [torch.randint(0, shape.vocab, (n,), generator=g).to(DEV) for n in lengths]
        bd = dec.batched(B)
        passes = plan_ragged_passes([n - 1 for n in lengths], 512)
        print(f"B {B:2d}: lengths {lengths}", flush=True)
        print(f"B {B:2d}: {sum(lengths) - B} prompt rows: {B} fill_slot passes against {len(passes)} ragged passes "
              f"(rows {[sum(r for _, _, r in p) for p in passes]})", flush=True)

        def loop():
            for b, pr in enumerate(prompts):
                bd.fill_slot(b, pr)

        def ragged():
            bd.fill_slots(range(B), prompts)
        # the same state behind both: positions and tokens exact, the first decode step within the tolerance
        loop()
        pos_ref, tok_ref = bd.pos.clone(), bd.tok.clone()
        ref = bd.step().float().clone()
        bd.reset()
        ragged()
        assert torch.equal(bd.pos, pos_ref) and torch.equal(bd.tok, tok_ref), "fill_slots left other positions / tokens"
        got = bd.step().float()
        err, tol = float((got - ref).abs().max()), 0.03 * (float(ref.abs().max()) + 1.0)
        assert err <= tol, f"B {B}: first-step logits differ by {err} (tolerance {tol})"
        agree = int((got.argmax(1) == ref.argmax(1)).sum())
        print(f"B {B:2d}: first decode step agrees, max diff {err:.4f} (tolerance {tol:.4f}), {agree} of {B} greedy tokens equal",
              flush=True)
        loop()            # the warm-up round (both routes ran once above already)
        ragged()
        res = {"loop": ([], []), "ragged": ([], [])}
        for _ in range(ROUNDS):
            for name, fn in (("loop", loop), ("ragged", ragged)):
                w, d = timed(fn)
                res[name][0].append(w)
                res[name][1].append(d)
        for name, label in (("loop", f"{B} x fill_slot"), ("ragged", "1 x fill_slots")):
            print(f"B {B:2d}: {label:15s} wall   {fmt(res[name][0])}", flush=True)
            print(f"B {B:2d}: {label:15s} device {fmt(res[name][1])}", flush=True)
        lw, rw = min(res["loop"][0]), min(res["ragged"][0])
        print(f"B {B:2d}: wall, best of {ROUNDS}: loop / ragged = {lw / rw:.2f}", flush=True)
        del bd
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
