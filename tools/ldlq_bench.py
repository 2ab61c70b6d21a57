"""What the panel route of quant.LDLQ buys at quantise time: QUIP.quant of one random nn.Linear at the 7B shapes
(4096 x 4096, 4096 -> 11008, 11008 -> 4096) with quip_tune_iters 0 and 10, the fused route (one GEMM + one ldlq_panel launch
per panel) and the stepwise route (QUIP_LDLQ_FUSED=0: one chain of launches per 8 columns) alternating in one process; wall
time of the whole call and of LDLQ inside it, medians of `--rounds` rounds with their spreads.  Then one 7B-shaped decoder
block (random fp16 weights) through QuipQuantizer.quantize_model on both routes.  One JSON line per measurement.
--codebook E8P12RVQ4B / E8P12RVQ3B measures the same for a residual codebook, whose fused route (ldlq_panel_rvq) sits behind
QUIP_LDLQ_FUSED_RVQ: the tool sets the route per call, so the stepwise route it alternates with is what LDLQ does by default.

    python tools/ldlq_bench.py [--codebook E8P12] [--rounds 3] [--tokens 2048] [--block-iters 10] [--skip-block] [--out FILE]"""
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
    ap.add_argument("--codebook", default="E8P12", choices=["E8P12", "E8P12RVQ4B", "E8P12RVQ3B"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tokens", type=int, default=2048)
    ap.add_argument("--block-iters", type=int, default=10)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--shapes", default="4096x4096,4096x11008,11008x4096")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ldlq_bench: needs a GPU (there is no CPU path to time)")
    import quip_for_all_amd as Q
    from quip_for_all_amd import quant, quip
    from quip_for_all_amd.quantizer import QuipQuantizer
    dev = "cuda:0"
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    ldlq_s = []
    ldlq0 = quip.LDLQ

    def timed_ldlq(*a, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = ldlq0(*a, **kw)
        torch.cuda.synchronize()
        ldlq_s.append(time.perf_counter() - t0)
        return r
    quip.LDLQ = timed_ldlq

    def set_route(route):
        """the process-wide switches quant.ldlq_route reads, set as their environment variables would set them"""
        if args.codebook == "E8P12":
            quant._LDLQ_FUSED = route == "fused"
        else:
            quant._LDLQ_FUSED, quant._LDLQ_FUSED_RVQ = True, route == "fused"
    emit(dict(device=torch.cuda.get_device_name(0), codebook=args.codebook, calibration_tokens=args.tokens, rounds=args.rounds,
              timing="host wall clock around synchronised calls; routes alternate inside every round"))
    cb = Q.codebook.codebook_id[args.codebook](inference=False).to(dev)
    for shape in args.shapes.split(","):
        fin, fout = (int(v) for v in shape.split("x"))
        torch.manual_seed(fin + fout)
        lin = torch.nn.Linear(fin, fout, bias=False).to(dev)
        W0 = lin.weight.data.clone()
        mix = torch.eye(fin, device=dev) + 0.3 * torch.randn(fin, fin, device=dev) / fin ** 0.5
        calib = (torch.randn(args.tokens, fin, device=dev) @ mix)[None]
        q = quip.QUIP(lin, cb)
        q.add_batch(calib)
        del mix, calib
        for iters in (0, 10):
            total = {"fused": [], "stepwise": []}
            inner = {"fused": [], "stepwise": []}
            rel = {}
            for rnd in range(args.rounds + 1):                       # round 0 warms both routes up and is dropped
                for route in ("fused", "stepwise"):
                    set_route(route)
                    assert quant.ldlq_route(W0.float(), cb) == ("panels" if route == "fused" else "stepwise")
                    lin.weight.data.copy_(W0)
                    torch.manual_seed(7)
                    del ldlq_s[:]
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    q.quant(quip_tune_iters=iters)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if rnd:
                        total[route].append(dt)
                        inner[route].append(ldlq_s[0])
                    rel[route] = ((lin.weight.data - W0).norm() / W0.norm()).item()
            rec = dict(linear=f"{fin}->{fout}", rows=fout, columns=fin, quip_tune_iters=iters)
            for route in total:
                rec[route] = dict(quant_s=[round(v, 4) for v in total[route]],
                                  quant_median_s=round(statistics.median(total[route]), 4),
                                  ldlq_median_s=round(statistics.median(inner[route]), 4),
                                  ldlq_spread_s=round(max(inner[route]) - min(inner[route]), 4),
                                  rel_error=round(rel[route], 4))
            rec["ldlq_speedup"] = round(rec["stepwise"]["ldlq_median_s"] / rec["fused"]["ldlq_median_s"], 2)
            rec["quant_speedup"] = round(rec["stepwise"]["quant_median_s"] / rec["fused"]["quant_median_s"], 2)
            emit(rec)
        q.free()
        del q, lin, W0
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
                   quip_tune_iters=args.block_iters, what="QuipQuantizer.quantize_model, whole call, once per route")
        for route in ("fused", "stepwise"):
            set_route(route)
            model = copy.deepcopy(base)
            qz = QuipQuantizer(codebook=args.codebook, dataset=data, nsamples=8, model_seqlen=512, batch_size=4,
                               quip_tune_iters=args.block_iters, ft_epochs=0)
            del ldlq_s[:]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            qz.quantize_model(model, None)
            torch.cuda.synchronize()
            rec[route] = dict(quantize_model_s=round(time.perf_counter() - t0, 3), ldlq_s=round(sum(ldlq_s), 3),
                              linears=len(ldlq_s))
            del model
            torch.cuda.empty_cache()
        rec["ldlq_speedup"] = round(rec["stepwise"]["ldlq_s"] / rec["fused"]["ldlq_s"], 2)
        rec["quantize_model_speedup"] = round(rec["stepwise"]["quantize_model_s"] / rec["fused"]["quantize_model_s"], 2)
        emit(rec)
    quip.LDLQ = ldlq0
    quant._LDLQ_FUSED = quant._LDLQ_FUSED_RVQ = None
    if out:
        out.close()


if __name__ == "__main__":
    main()
