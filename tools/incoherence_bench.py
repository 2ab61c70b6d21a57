"""What the fused incoherence transforms buy at quantise time: quant.incoherence_in + quant.incoherence_out of one
(rows <- columns) layer with QUIP_INCOHERENCE_FUSED on (two had_wide_rows launches per matrix, csrc/had_wide.hip) and off (the
torch expressions), alternating in one process after a warm-up round.  A timing is device events around enough calls to fill
`--window` seconds; per route the median and the spread of `--rounds` timings and the largest difference of the two results
relative to max |.|.  Then the transposed store alone, H (n, n) -> H^T-side of one launch, with and without the XCD swizzle of
the row tiles: achieved bytes/s from the shapes (n^2 read, n^2 written).  Then one 7B-shaped decoder block (random fp16
weights) through QuipQuantizer.quantize_model with the switch off and on.  One JSON line per measurement.

    python tools/incoherence_bench.py [--rounds 5] [--window 0.3] [--skip-block] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 4096, "float32"), (4096, 11008, "float32"), (11008, 4096, "float32"), (8192, 28672, "float32"),
          (4096, 4096, "float64")]                                # (columns, rows, dtype): columns -> rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--block-iters", type=int, default=10)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("incoherence_bench: needs a GPU (there is no CPU path to time)")
    from quip_for_all_amd import capi, quant
    from quip_for_all_amd.quantizer import QuipQuantizer
    dev = "cuda:0"
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    def timed(fn, reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        return start.elapsed_time(stop) / 1e3 / reps

    def compare(calls):
        """{name: fn} -> {name: dict(median_ms, spread_ms, calls_per_timing)}, the routes alternating inside every round"""
        reps, secs = {}, {k: [] for k in calls}
        for k, fn in calls.items():                                # warm-up, and how many calls fill the window
            fn()
            reps[k] = max(1, int(args.window / timed(fn, 1)))
        for _ in range(args.rounds):
            for k, fn in calls.items():
                secs[k].append(timed(fn, reps[k]))
        return {k: dict(calls_per_timing=reps[k], median_ms=round(statistics.median(v) * 1e3, 3),
                        spread_ms=round((max(v) - min(v)) * 1e3, 3)) for k, v in secs.items()}

    def verdict(rec, slow, fast):
        rec["speedup"] = round(rec[slow]["median_ms"] / rec[fast]["median_ms"], 2)
        rec["difference_over_twice_larger_spread"] = round(
            (rec[slow]["median_ms"] - rec[fast]["median_ms"]) / max(2 * max(rec[slow]["spread_ms"], rec[fast]["spread_ms"]), 1e-6), 1)

    emit(dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window,
              timing="device events around `reps` calls of incoherence_in + incoherence_out; routes alternate inside every round"))
    for columns, rows, dname in SHAPES:
        dtype = getattr(torch, dname)
        torch.manual_seed(columns + rows)
        (lhad, lK, lN), (rhad, rK, rN) = quant.get_hadK(columns), quant.get_hadK(rows)
        H = torch.randn(columns, columns, device=dev, dtype=dtype)
        w = torch.randn(rows, columns, device=dev, dtype=dtype)
        SU, SV = (torch.randn(k, device=dev).sign().to(dtype) for k in (columns, rows))
        side = (lhad, lK, lN, rhad, rK, rN)
        res = {}

        def call(route):
            quant._INCOHERENCE_FUSED = route == "fused"
            Hi, wi = quant.incoherence_in(H, w, SU, SV, *side)
            res[route] = (Hi, wi, quant.incoherence_out(wi, SU, SV, *side, columns, rows))
        quant._INCOHERENCE_FUSED = True
        rec = dict(columns=columns, rows=rows, dtype=dname, left=(lK, lN // lK), right=(rK, rN // rK),
                   fused_route=quant.incoherence_route(H, lK, lN, rK, rN))
        rec.update(compare({"fused": lambda: call("fused"), "torch": lambda: call("torch")}))
        rec["max_rel_diff"] = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(res["fused"], res["torch"]))
        verdict(rec, "torch", "fused")
        emit(rec)
        del res, H, w
        torch.cuda.empty_cache()
    quant._INCOHERENCE_FUSED = None

    for n, K in ((4096, 1), (11008, 43)):                          # the transposed store, with and without the XCD swizzle
        x = torch.randn(n, n, device=dev)
        y = torch.empty(n, n, device=dev)
        hadK = None if K == 1 else quant.get_hadK(n)[0].to(dev).contiguous()
        stream = torch.cuda.current_stream().cuda_stream

        def launch(swizzle):
            capi.check(capi.lib().quip_had_wide_rows_tuned(y.data_ptr(), x.data_ptr(), 2, n, n, n, n, K, None if K == 1 else
                                                           hadK.data_ptr(), 1, None, None, 1.0, 1, swizzle, stream), "tuned")
        rec = dict(transposed_store=n, K=K, dtype="float32", bytes=2 * 4 * n * n)
        rec.update(compare({"swizzle": lambda: launch(1), "plain": lambda: launch(0)}))
        for k in ("swizzle", "plain"):
            rec[k]["achieved_GBps"] = round(rec["bytes"] / rec[k]["median_ms"] / 1e6, 1)
        verdict(rec, "plain", "swizzle")
        emit(rec)
        del x, y
        torch.cuda.empty_cache()

    if not args.skip_block:
        import copy
        from transformers import AutoModelForCausalLM, LlamaConfig
        cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=1, num_attention_heads=32,
                          vocab_size=32000, max_position_embeddings=2048, tie_word_embeddings=False)
        torch.manual_seed(1)
        base = AutoModelForCausalLM.from_config(cfg, dtype=torch.float16)
        g = torch.Generator().manual_seed(2)
        data = [torch.randint(0, 32000, (512,), generator=g) for _ in range(8)]
        rec = dict(block="Llama-2-7B-shaped, 1 layer, random fp16 weights", calibration="8 x 512 random tokens, batch_size 4",
                   quip_tune_iters=args.block_iters, what="QuipQuantizer.quantize_model, whole call, host clock, synchronised")
        secs = {"off": [], "on": []}
        for route in ("off", "on", "off", "on", "off", "on"):       # the first pair warms both routes up
            quant._INCOHERENCE_FUSED = route == "on"
            model = copy.deepcopy(base)
            qz = QuipQuantizer(codebook="E8P12", dataset=data, nsamples=8, model_seqlen=512, batch_size=4,
                               quip_tune_iters=args.block_iters, ft_epochs=0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qz.quantize_model(model, None)
            torch.cuda.synchronize()
            secs[route].append(round(time.perf_counter() - t0, 3))
            del model
            torch.cuda.empty_cache()
        rec["quantize_model_s"] = {k: v[1:] for k, v in secs.items()}
        emit(rec)
        quant._INCOHERENCE_FUSED = None
    if out:
        out.close()


if __name__ == "__main__":
    main()
