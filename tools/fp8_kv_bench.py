"""The fp8 (e4m3fn) paged KV cache against the fp16 paged one on the 7B-shaped random decoder (E8P12), B = 16.

Both decoders live in one process on the same modules; after warm-up replays of both, --rounds rounds alternate them
and the figure to read is the fp8 / fp16 ratio of the medians next to the spread of the rounds (min .. max of each side):
a difference inside that spread is not a difference.

  1. the attention launch alone, both ways, through captured graphs at --long-pos and at 256: the fp8 launch streams
     half the cache bytes through the same shuffled block table;
  2. the captured step at short context (positions from 16) and from --long-pos.

One JSON line per measurement on stdout; --out appends them, with a header, to a profile file.

    python tools/fp8_kv_bench.py [--steps 48] [--rounds 5] [--long-pos 2048] [--out profiles/fp8_kv_bench.txt]"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = 16
SIDES = ("fp16", "fp8")


def _replays(graph, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        graph.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _summary(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def _alternate(name, fp16, fp8, args):
    """fp16 / fp8: (graph, reset) -> one result line"""
    for graph, reset in (fp16, fp8):
        reset()
        _replays(graph, args.warmup)
    ms = {k: [] for k in SIDES}
    for _ in range(args.rounds):
        for key, (graph, reset) in zip(SIDES, (fp16, fp8)):
            reset()
            ms[key].append(_replays(graph, args.steps))
    res = {"what": name, "unit": "ms per replay", "rounds": args.rounds, "replays_per_round": args.steps,
           "fp16": _summary(ms["fp16"]), "fp8": _summary(ms["fp8"])}
    res["fp8_over_fp16"] = round(res["fp8"]["median"] / res["fp16"]["median"], 4)
    for k in SIDES:
        res[f"spread_{k}"] = round(res[k]["max"] / res[k]["min"] - 1, 4)
    return res


def bench_attention(args, emit, P):
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.paged_attn as PA
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    heads, kvh, hd, dev = 32, 32, 128, "cuda:0"
    max_pages = P // 64 + 1
    max_len = max_pages * 64
    ids = list(range(B * max_pages))
    random.Random(0).shuffle(ids)
    table = torch.tensor(ids, dtype=torch.int32, device=dev).view(B, max_pages)
    # the fp16 pools hold what the fp8 bytes mean: both launches compute with the same cached values
    codes = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f], dtype=torch.uint8, device=dev)
    lut = PA.dequant_f8(torch.arange(256, dtype=torch.uint8), -4).to(dev)
    pools8 = [codes[torch.randint(0, 254, (B * max_pages, kvh, 64, hd), device=dev)] for _ in range(2)]
    pools16 = [lut[p.long()] for p in pools8]
    q = torch.randn(B, heads, hd, device=dev).half()
    k, v = torch.randn(B, kvh, hd, device=dev).half(), torch.randn(B, kvh, hd, device=dev).half()
    ang = torch.rand(max_len, hd, device=dev) * 6.283
    cos, sin = ang.cos(), ang.sin()
    pos = torch.full((B,), P, dtype=torch.long, device=dev)
    ws = [rope_attn_batched_workspace(B, heads, hd, dev) for _ in range(2)]
    graphs = []
    for fn in (lambda: torch.ops.quip_lib.rope_attn_decode_paged(q, k, v, cos, sin, pos, table, pools16[0], pools16[1], ws[0], 0),
               lambda: torch.ops.quip_lib.rope_attn_decode_paged_f8(q, k, v, cos, sin, pos, table, pools8[0], pools8[1], ws[1], 0,
                                                                    -4, -4)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.attn_launches):
                fn()
        graphs.append(g)
    r = _alternate(f"attention_launch_alone_pos{P}", (graphs[0], lambda: None), (graphs[1], lambda: None), args)
    r.update({"shape": f"B={B} heads={heads} kv_heads={kvh} hd={hd} positions={P + 1}", "launches_per_replay": args.attn_launches})
    for key, width in zip(SIDES, (2, 1)):
        nbytes = B * 2 * kvh * (P + 1) * hd * width
        us = r[key]["median"] * 1e3 / args.attn_launches
        r[f"us_per_launch_{key}"] = round(us, 2)
        r[f"cache_bytes_per_launch_{key}"] = nbytes
        r[f"cache_TBps_{key}"] = round(nbytes / (us * 1e-6) / 1e12, 3)
    emit(r)


def bench_steps(args, emit):
    from quip_for_all_amd import decode as D
    max_len = args.long_pos + args.steps + args.warmup + 16
    dec = D.LlamaDecoder(D.LLAMA2_7B, "E8P12", max_len=max_len, device="cuda:0", seed=0, device_init=True)
    decs = {"fp16": dec.batched(B, paged=True), "fp8": dec.batched(B, paged=True, kv_dtype="fp8")}
    for d in decs.values():
        d.capture()
        # every slot holds all its pages, handed out in a shuffled order: the step reads a scattered cache
        ids = list(range(d.n_pages))
        random.Random(0).shuffle(ids)
        d.pool.free = ids
        for b in range(B):
            d.pool.reserve(b, max_len)
        d._push_table()
    tok = torch.randint(0, dec.s.vocab, (B,), generator=torch.Generator().manual_seed(1)).to("cuda:0")
    s = dec.s
    page = 2 * s.layers * s.kv_heads * 64 * s.head_dim
    emit({"what": "setup", "batch": B, "max_len": max_len, "pages": decs["fp16"].n_pages,
          "page_MB_all_layers": {"fp16": round(page * 2 / 2 ** 20, 1), "fp8": round(page / 2 ** 20, 1)},
          "pages_per_GB": {"fp16": 2 ** 30 // (page * 2), "fp8": 2 ** 30 // page},
          "pool_GB": {k: round(2 * d.kpool.numel() * d.kpool.element_size() / 2 ** 30, 2) for k, d in decs.items()}})
    for name, p0 in (("step_short", 16), ("step_long", args.long_pos)):
        def reset(d):
            d.pos.fill_(p0)
            d.tok.copy_(tok)
        r = _alternate(name, (decs["fp16"].graph, lambda: reset(decs["fp16"])), (decs["fp8"].graph, lambda: reset(decs["fp8"])),
                       args)
        r["positions"] = [p0, p0 + args.steps]
        for k in SIDES:
            r[f"tok_s_{k}"] = round(B * 1e3 / r[k]["median"], 1)
        emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long-pos", type=int, default=2048)
    ap.add_argument("--attn-launches", type=int, default=32, help="attention launches per captured graph")
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--out", default=None, help="append the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_kv_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    with torch.no_grad():
        for P in (args.long_pos, 256):
            bench_attention(args, emit, P)
            torch.cuda.empty_cache()
        if not args.attn_only:
            bench_steps(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write("# tools/fp8_kv_bench.py: fp8 (e4m3fn) against fp16 paged KV cache, 7B shape, E8P12, B = 16, captured graphs,\n"
                    "# device events; fp16 and fp8 alternate round by round in one process after warm-up replays.\n"
                    "# spread_* = max / min - 1 over the rounds of one side: an fp8_over_fp16 inside it is no difference.\n"
                    f"# device: {torch.cuda.get_device_name(0)}; arguments: {vars(args)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
