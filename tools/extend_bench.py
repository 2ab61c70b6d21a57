#!/usr/bin/env python3
"""The chunked prompt pass (LlamaDecoder.extend: one rope_attn_chunk launch per block and chunk) on the 32-layer 7B decoder:

  (a) from position 0 against prefill() at P = 64 / 512 / 2048 -- the logits of the two passes are compared first
      (0.03 (max|ref| + 1), the tolerance of the prompt-pass tests), then both are timed (P = 2048 also as ONE chunk:
      the default chunk of 512 rows bounds the activations and pays for it by running every product four times);
  (b) appending 256 tokens at position 1024: extend() and extend_graph() against 256 replays of the captured step, the
      only way to do that before extend() existed.

Device events, two warm-up runs, three repetitions each (all printed: the spread is part of the answer), best of 3.

  --baseline-only     prefill() and the step replays only (runs on a tree without extend())
  --pass NAME P       one warmed-up pass of NAME (prefill | extend) over P tokens and nothing else: the run to put under
                      rocprofv3 --kernel-trace --stats"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402

DEV = "cuda:0"
MAX_LEN = 2304


def timed(fn, prepare, reps=3, warmup=2):
    """milliseconds of fn() (device events), `prepare()` before every run -> list of `reps` times"""
    with torch.no_grad():
        for _ in range(warmup):
            prepare()
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            prepare()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            out.append(a.elapsed_time(b))
    return out


def fmt(ts):
    return f"best {min(ts):9.2f} ms   (runs " + " ".join(f"{t:.2f}" for t in ts) + f"; spread {max(ts) - min(ts):.2f})"


def main():
    baseline = "--baseline-only" in sys.argv
    dec = D.LlamaDecoder(D.LLAMA2_7B, "E8P12", max_len=MAX_LEN, device=DEV, device_init=True)
    g = torch.Generator().manual_seed(0)
    toks = lambda n: torch.randint(0, dec.s.vocab, (n,), generator=g).to(DEV)  # noqa: E731
    if "--pass" in sys.argv:
        name, P = sys.argv[sys.argv.index("--pass") + 1], int(sys.argv[sys.argv.index("--pass") + 2])
        t = toks(P)
        with torch.no_grad():
            for _ in range(2):
                dec.reset()
                getattr(dec, name)(t)
        torch.cuda.synchronize()
        print(f"{name} over {P} tokens: done", flush=True)
        return
    dec.capture()                                   # first: its warm-up steps write cache rows 0 and 1
    print(f"7B E8P12, max_len {MAX_LEN}" + (" -- baseline only" if baseline else ""), flush=True)
    for P in (64, 512, 2048):
        t = toks(P)
        if not baseline:
            with torch.no_grad():
                dec.reset()
                ref = dec.prefill(t).float()
                dec.reset()
                got = dec.extend(t).float()
            err, tol = float((got - ref).abs().max()), 0.03 * (float(ref.abs().max()) + 1.0)
            assert err <= tol, f"P {P}: extend and prefill logits differ by {err} (tolerance {tol})"
            print(f"from 0, P {P:5d}: logits agree, max diff {err:.4f} (tolerance {tol:.4f})", flush=True)
        print(f"from 0, P {P:5d}: prefill      {fmt(timed(lambda: dec.prefill(t), dec.reset))}", flush=True)
        if not baseline:
            print(f"from 0, P {P:5d}: extend       {fmt(timed(lambda: dec.extend(t), dec.reset))}", flush=True)
            if P > 512:     # the default chunk of 512 rows repeats every product per chunk; the whole prompt as one chunk:
                print(f"from 0, P {P:5d}: extend, chunk = P {fmt(timed(lambda: dec.extend(t, chunk=P), dec.reset))}", flush=True)
    # (b) 256 tokens behind 1024 cached ones
    hist, more = toks(1024), toks(256)
    with torch.no_grad():
        dec.reset()
        dec.prefill(hist)

    def at_1024():
        dec.pos.fill_(1024)
        dec.tok.copy_(more[:1])

    def steps():
        for _ in range(256):
            dec.graph.replay()
    print(f"append 256 @ 1024: 256 step replays {fmt(timed(steps, at_1024))}", flush=True)
    if not baseline:
        print(f"append 256 @ 1024: extend           {fmt(timed(lambda: dec.extend(more), at_1024))}", flush=True)
        print(f"append 256 @ 1024: extend_graph     {fmt(timed(lambda: dec.extend_graph(more), at_1024))}", flush=True)
        with torch.no_grad():
            at_1024()
            a = dec.extend(more).clone()
            at_1024()
            b = dec.extend_graph(more)
        assert torch.equal(a, b), "extend_graph and extend disagree"
        print("append 256 @ 1024: extend_graph logits == extend logits (bit for bit)", flush=True)


if __name__ == "__main__":
    main()
