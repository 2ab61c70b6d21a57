"""q / k norm inside the attention launch against the stand-alone norm launch in front of it, on a Qwen3-8B-shaped random
decoder (hidden 4096, 32 / 8 heads, head_dim 128, 36 layers, vocab 151936, ffn 12288; E8P12, `LlamaDecoder(qk_norm=True)`).

Two captured steps of the SAME decoder -- `qk_fused` on (quip_lib::rope_attn_decode_qknorm / _batched_qknorm) and off
(quip_lib::qk_norm_rows + the plain launch: the same bits, one more launch per block) -- are replayed alternately in one
process and timed with device events: the bs = 1 step and the B = --batch step, at positions [16, 16 + K) and from
--long-pos.  One JSON line per (step, position range): ms per step of every round for both routes, their medians and the
difference.  --out also writes the lines to a file.

    python tools/qk_norm_bench.py [--steps 64] [--warmup 8] [--rounds 7] [--batch 16] [--long-pos 2048] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(replay, steps, warmup, reset):
    reset()
    for _ in range(warmup):
        replay()
    reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _two_graphs(parent, stepper):
    """the captured step of `stepper` (the decoder itself, or one of its batched decoders) with the norm fused and not"""
    graphs = {}
    for name, fused in (("fused", True), ("unfused", False)):
        parent.qk_fused, stepper.graph = fused, None
        stepper.capture()
        graphs[name] = stepper.graph
    parent.qk_fused = True
    return graphs


def _ab(what, graphs, reset_at, where, args, emit, extra):
    for name, p0 in where:
        ms = {"fused": [], "unfused": []}
        for _ in range(args.rounds):
            for route in ("fused", "unfused"):                   # alternating: both routes see the same machine
                ms[route].append(_time(graphs[route].replay, args.steps, args.warmup, lambda: reset_at(p0)))
        med = {r: statistics.median(v) for r, v in ms.items()}
        emit(dict(step=what, positions=[p0, p0 + args.steps], rounds=args.rounds, steps_per_round=args.steps,
                  ms_fused=[round(x, 4) for x in ms["fused"]], ms_unfused=[round(x, 4) for x in ms["unfused"]],
                  median_ms_fused=round(med["fused"], 4), median_ms_unfused=round(med["unfused"], 4),
                  unfused_minus_fused_us=round(1e3 * (med["unfused"] - med["fused"]), 2),
                  spread_us_fused=round(1e3 * (max(ms["fused"]) - min(ms["fused"])), 2),
                  spread_us_unfused=round(1e3 * (max(ms["unfused"]) - min(ms["unfused"])), 2), **extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--long-pos", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=36)
    ap.add_argument("--vocab", type=int, default=151936)
    ap.add_argument("--ffn", type=int, default=12288)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qk_norm_bench: needs a GPU (there is no CPU path to time)")
    from quip_for_all_amd import decode as D
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    shape = D.LlamaShape(hidden=4096, ffn=args.ffn, layers=args.layers, heads=32, kv_heads=8, vocab=args.vocab, rms_eps=1e-6,
                         rope_theta=1e6, head_dim=128)
    max_len = args.long_pos + args.steps + args.warmup + 16
    with torch.no_grad():
        dec = D.LlamaDecoder(shape, "E8P12", max_len=max_len, device="cuda:0", seed=0, device_init=True, qk_norm=True)
        emit(dict(model="Qwen3-8B-shaped random init", hidden=shape.hidden, ffn=shape.ffn, layers=shape.layers, heads=shape.heads,
                  kv_heads=shape.kv_heads, head_dim=shape.head_dim, vocab=shape.vocab, codebook="E8P12", max_len=max_len,
                  fused_prologue=bool(dec.fused_prologue), chain=bool(dec.chain), ffn_eng=bool(dec.ffn_eng),
                  block_eng=bool(dec.block_eng), attn_z=bool(dec.attn_z), device=torch.cuda.get_device_name(0)))
        where = (("short", 16), ("long", args.long_pos))
        g = torch.Generator(device="cuda:0").manual_seed(1)
        _ab("bs1", _two_graphs(dec, dec), lambda p0: dec.pos.fill_(p0), where, args, emit, {})
        dec.graph = None
        B = args.batch
        bd = dec.batched(B)

        def reset_at(p0):
            bd.pos.fill_(p0)
            bd.tok.copy_(torch.randint(0, shape.vocab, (B,), generator=g, device="cuda:0"))
        _ab(f"B{B}", _two_graphs(dec, bd), reset_at, where, args, emit, {"batch": B, "regimes": bd.regimes()})
    if out:
        out.close()


if __name__ == "__main__":
    main()
