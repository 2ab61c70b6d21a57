"""What the fused Hessian accumulation buys at quantise time: QUIP.add_batch of one (rows, n) activation with
QUIP_HESSIAN_FUSED on (one hessian_accumulate launch, csrc/hessian.hip) and off (the torch expression: fp64 copy, full fp64
GEMM, n x n temporary), alternating in one process after a warm-up round.  A timing is device events around enough calls to
fill `--window` seconds; per route the median and the spread of `--rounds` timings, the achieved fp64 operations per second
from the shapes (n (n + 1) rows for the launch, 2 n^2 rows for the GEMM) and the largest difference of the two results
relative to max |H|.  Then one 7B-shaped decoder block (random fp16 weights) through QuipQuantizer.quantize_model with the
switch off and on: the whole call and the time inside the forward hooks.  One JSON line per measurement.

    python tools/hessian_bench.py [--rounds 5] [--window 0.3] [--n 4096,11008] [--rows 4096,16384] [--skip-block] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--n", default="4096,11008")
    ap.add_argument("--rows", default="4096,16384")
    ap.add_argument("--block-iters", type=int, default=10)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hessian_bench: needs a GPU (there is no CPU path to time)")
    import quip_for_all_amd as Q
    from quip_for_all_amd import quip
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

    emit(dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, window_s=args.window,
              timing="device events around `reps` calls of QUIP.add_batch; routes alternate inside every round"))
    cb = Q.codebook.codebook_id["E8P12"](inference=False).to(dev)
    for n in (int(v) for v in args.n.split(",")):
        lin = torch.nn.Linear(n, 8, bias=False).to(dev)
        for rows in (int(v) for v in args.rows.split(",")):
            for dtype in (torch.float32, torch.float16):
                torch.manual_seed(n + rows)
                x = torch.randn(1, rows, n, device=dev).to(dtype)
                qs = {route: quip.QUIP(lin, cb) for route in ("fused", "torch")}

                def call(route):
                    quip._HESSIAN_FUSED = route == "fused"
                    qs[route].add_batch(x)
                reps, secs = {}, {"fused": [], "torch": []}
                for route in qs:                                         # warm-up, and how many calls fill the window
                    call(route)
                    reps[route] = max(1, int(args.window / timed(lambda: call(route), 1)))
                for _ in range(args.rounds):
                    for route in qs:
                        secs[route].append(timed(lambda: call(route), reps[route]))
                diff = ((qs["fused"].H - qs["torch"].H).abs().max() / qs["torch"].H.abs().max()).item()
                ops = {"fused": n * (n + 1) * rows, "torch": 2 * n * n * rows}
                rec = dict(n=n, rows=rows, dtype=str(dtype).split(".")[1], max_rel_diff=diff)
                for route in qs:
                    med = statistics.median(secs[route])
                    rec[route] = dict(calls_per_timing=reps[route], median_ms=round(med * 1e3, 3),
                                      spread_ms=round((max(secs[route]) - min(secs[route])) * 1e3, 3),
                                      fp64_tops=round(ops[route] / med / 1e12, 2))
                rec["speedup"] = round(rec["torch"]["median_ms"] / rec["fused"]["median_ms"], 2)
                rec["difference_over_twice_larger_spread"] = round(
                    (rec["torch"]["median_ms"] - rec["fused"]["median_ms"])
                    / max(2 * max(rec["torch"]["spread_ms"], rec["fused"]["spread_ms"]), 1e-6), 1)
                emit(rec)
                for q in qs.values():
                    q.free()
                del qs, x
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
                   quip_tune_iters=args.block_iters, what="QuipQuantizer.quantize_model, whole call, once per route; hooks_s: "
                   "host wall clock around the synchronised forward hooks (accumulations and copies)")
        hook_s, copies = [], []
        plain, shared = quip.QUIP.add_batch, quip.SharedHessianInputs.add_batch

        def clocked(fn, outer):
            def run(self, *a, **kw):
                if not outer():
                    return fn(self, *a, **kw)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(self, *a, **kw)
                torch.cuda.synchronize()
                hook_s.append(time.perf_counter() - t0)
                if isinstance(self, quip.SharedHessianInputs):
                    copies[:] = [self.copies]
            return run
        quip.QUIP.add_batch = clocked(plain, lambda: not quip._HESSIAN_FUSED)       # inside the shared hook when on
        quip.SharedHessianInputs.add_batch = clocked(shared, lambda: True)
        for route in ("off", "on", "off", "on"):                                    # the first pair warms both routes up
            quip._HESSIAN_FUSED = route == "on"
            model = copy.deepcopy(base)
            qz = QuipQuantizer(codebook="E8P12", dataset=data, nsamples=8, model_seqlen=512, batch_size=4,
                               quip_tune_iters=args.block_iters, ft_epochs=0)
            del hook_s[:], copies[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qz.quantize_model(model, None)
            torch.cuda.synchronize()
            rec[route] = dict(quantize_model_s=round(time.perf_counter() - t0, 3), hooks_s=round(sum(hook_s), 4),
                              hook_calls=len(hook_s), copies=sum(copies))
            del model
            torch.cuda.empty_cache()
        quip.QUIP.add_batch, quip.SharedHessianInputs.add_batch = plain, shared
        rec["hooks_speedup"] = round(rec["off"]["hooks_s"] / rec["on"]["hooks_s"], 2)
        emit(rec)
    quip._HESSIAN_FUSED = None
    if out:
        out.close()


if __name__ == "__main__":
    main()
