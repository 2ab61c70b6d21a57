"""HF `generate` on a left-padded batch: the stock forward against hf_fast's batch route, in one process.

The 7B-shaped random HF model (E8P12; tests/test_gpu_hf_generate.py::_random_quantized_hf_llama), B = 16 prompts of
fixed-seed lengths in [24, 200], left padded, 64 new tokens, greedy, the default DynamicCache.  After one warm-up round
of each route (code objects, the decoder and its buffers, library heuristics) the two routes ALTERNATE for --rounds
rounds; every generation is timed with a host clock around work that ends in a device synchronise.  Printed: one JSON line
per generation, then one summary line with the medians of wall time and tokens per second (new tokens of all sequences /
wall time, prompt pass included: it is the stock forward in both routes) and the route's step counters.  The prompt pass
alone is timed once per route too, so that the decode share can be read off.

    python tools/hf_batch_generate_bench.py [--batch 16] [--new 64] [--rounds 3] [--layers 32]"""
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
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--new", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--max-pos", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hf_batch_generate_bench: needs a GPU (nothing is measured without one)")
    from transformers import LlamaConfig
    from quip_for_all_amd.hf_fast import enable_fast_decode
    from tests.test_gpu_hf_generate import _random_quantized_hf_llama
    cfg = LlamaConfig(hidden_size=4096, intermediate_size=11008, num_hidden_layers=args.layers, num_attention_heads=32,
                      num_key_value_heads=32, vocab_size=32000, max_position_embeddings=args.max_pos, rms_norm_eps=1e-5,
                      tie_word_embeddings=False)
    model = _random_quantized_hf_llama(cfg)
    model.generation_config.eos_token_id = None
    model.generation_config.pad_token_id = 0
    g = torch.Generator().manual_seed(1234)
    lengths = torch.randint(24, 201, (args.batch,), generator=g).tolist()
    width = max(lengths)
    ids = torch.zeros(args.batch, width, dtype=torch.long)
    mask = torch.zeros(args.batch, width, dtype=torch.long)
    for b, n in enumerate(lengths):
        ids[b, width - n:] = torch.randint(1, cfg.vocab_size, (n,), generator=g)
        mask[b, width - n:] = 1
    ids, mask = ids.to("cuda:0"), mask.to("cuda:0")

    def generate(new):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = model.generate(ids, attention_mask=mask, max_new_tokens=new, do_sample=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out[:, width:]

    enable_fast_decode(model, batch=True)
    fd = model._quip_fast_decode           # one wrapper for the whole run: its decoder and buffers are built once, in the warm-up

    def run(route, new):
        model.forward = fd if route == "batch" else fd.orig_forward
        return generate(new)
    print(json.dumps({"what": "setup", "batch": args.batch, "lengths": lengths, "new_tokens": args.new, "layers": args.layers,
                      "device": torch.cuda.get_device_name(0)}), flush=True)
    for route in ("stock", "batch"):       # warm-up round
        s, _ = run(route, args.new)
        print(json.dumps({"what": "warmup", "route": route, "wall_s": round(s, 4)}), flush=True)
    wall, prompt, toks = {"stock": [], "batch": []}, {}, {}
    for r in range(args.rounds):
        for route in ("stock", "batch"):
            s, t = run(route, args.new)
            wall[route].append(s)
            toks[route] = t
            print(json.dumps({"what": "round", "round": r, "route": route, "wall_s": round(s, 4),
                              "tok_s": round(args.batch * args.new / s, 1)}), flush=True)
    for route in ("stock", "batch"):       # the prompt pass and the first token alone
        prompt[route] = min(run(route, 1)[0] for _ in range(2))
    agree = float((toks["stock"] == toks["batch"]).float().mean())
    res = {"what": "summary", "batch": args.batch, "new_tokens": args.new}
    for route in ("stock", "batch"):
        med = statistics.median(wall[route])
        res[route + "_route"] = {"median_wall_s": round(med, 4), "min_wall_s": round(min(wall[route]), 4),
                      "max_wall_s": round(max(wall[route]), 4), "tok_s": round(args.batch * args.new / med, 1),
                      "tok_s_per_seq": round(args.new / med, 1), "prompt_pass_s": round(prompt[route], 4),
                      "decode_tok_s": round(args.batch * (args.new - 1) / max(med - prompt[route], 1e-9), 1)}
    res["speedup_wall"] = round(res["stock_route"]["median_wall_s"] / res["batch_route"]["median_wall_s"], 3)
    res["speedup_decode"] = round(res["batch_route"]["decode_tok_s"] / res["stock_route"]["decode_tok_s"], 3)
    res["fast_batch_steps"], res["batch_imports"], res["batch_disabled"] = fd.fast_batch_steps, fd.batch_imports, fd.batch_disabled
    res["greedy_tokens_equal_share"] = round(agree, 4)      # (random weights: near ties fork the routes; not a parity check)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
