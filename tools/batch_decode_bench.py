"""Batched decode on the 7B-shaped random decoder (E8P12): captured BatchDecoder steps for B in --batches, timed with
device events at positions [16, 16 + K) and at --long-pos, one JSON line per B (ms per step, aggregate tok/s, tok/s per
sequence, the regime every module takes at M = B).  The parent decoder's own captured bs=1 step is timed the same way
first (the bs=1 headline path).  --attn: the batched attention launch alone at B = 16 / --long-pos positions against
B single-sequence launches, with the cache bytes read per second.

    python tools/batch_decode_bench.py [--batches 1,2,4,8,16,31] [--steps 64] [--warmup 8] [--attn]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _time(fn, steps, warmup, reset):
    reset()
    for _ in range(warmup):
        fn()
    reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def bench_steps(args):
    from quip_for_all_amd import decode as D
    max_len = args.long_pos + args.steps + args.warmup + 16
    dec = D.LlamaDecoder(D.LLAMA2_7B, "E8P12", max_len=max_len, device="cuda:0", seed=0, device_init=True)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    where = (("short", 16),) if args.short_only else (("short", 16), ("long", args.long_pos))
    if not args.skip_bs1:
        dec.capture()
        res = {"batch": "bs1_parent", "block_eng": bool(dec.block_eng)}
        for name, p0 in where:
            ms = _time(dec.graph.replay, args.steps, args.warmup, lambda: dec.pos.fill_(p0))
            res[f"ms_per_step_{name}"] = round(ms, 4)
            res[f"tok_s_{name}"] = round(1e3 / ms, 1)
        print(json.dumps(res), flush=True)
    for B in args.batches:
        bd = dec.batched(B)
        bd.capture()
        res = {"batch": B, "regimes": bd.regimes()}
        for name, p0 in where:
            def reset():
                bd.pos.fill_(p0)
                bd.tok.copy_(torch.randint(0, dec.s.vocab, (B,), generator=g, device="cuda:0"))
            ms = _time(bd.graph.replay, args.steps, args.warmup, reset)
            res[f"ms_per_step_{name}"] = round(ms, 4)
            res[f"tok_s_{name}"] = round(B * 1e3 / ms, 1)
            res[f"tok_s_per_seq_{name}"] = round(1e3 / ms, 1)
        res["positions_short"] = [16, 16 + args.steps]
        if not args.short_only:
            res["positions_long"] = [args.long_pos, args.long_pos + args.steps]
        print(json.dumps(res), flush=True)
        del bd
        torch.cuda.empty_cache()


def bench_attention(args):
    import quip_for_all_amd  # noqa: F401
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    from quip_for_all_amd.register_lib import rope_attn_workspace
    B, heads, kvh, hd, P = 16, 32, 32, 128, args.long_pos
    max_len = P + 1
    dev = "cuda:0"
    kc = torch.randn(B, kvh, max_len, hd, device=dev).half()
    vc = torch.randn_like(kc)
    q = torch.randn(B, heads, hd, device=dev).half()
    k, v = torch.randn(B, kvh, hd, device=dev).half(), torch.randn(B, kvh, hd, device=dev).half()
    cos, sin = torch.randn(max_len, hd, device=dev), torch.randn(max_len, hd, device=dev)
    pos = torch.full((B,), P, dtype=torch.long, device=dev)
    wsb = rope_attn_batched_workspace(B, heads, hd, dev)
    ws1 = [rope_attn_workspace(heads, hd, dev) for _ in range(B)]

    def batched():
        torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, cos, sin, pos, kc, vc, wsb, 0)

    def singles():
        for b in range(B):
            torch.ops.quip_lib.rope_attn_decode(q[b], k[b], v[b], cos, sin, pos[b:b + 1], kc[b], vc[b], ws1[b], 0)
    # launched through captured graphs, as in the decode step (no host launch overhead in the timing)
    res = {"attention": f"B={B} heads={heads} kv_heads={kvh} hd={hd} positions={P + 1}"}
    nbytes = B * 2 * kvh * (P + 1) * hd * 2
    for name, fn in (("batched", batched), ("singles", singles)):
        fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            fn()
        ms = _time(gr.replay, args.attn_reps, 5, lambda: None)
        res[f"us_{name}"] = round(ms * 1e3, 2)
        res[f"cache_TBps_{name}"] = round(nbytes / (ms * 1e-3) / 1e12, 3)
    res["cache_bytes"] = nbytes
    res["fraction_of_8TBps_batched"] = round(res["cache_TBps_batched"] / 8.0, 3)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,2,4,8,16,31")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--long-pos", type=int, default=2048)
    ap.add_argument("--attn", action="store_true", help="time the batched attention launch against single launches")
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--attn-reps", type=int, default=50)
    ap.add_argument("--skip-bs1", action="store_true", help="do not time the parent's bs=1 step")
    ap.add_argument("--short-only", action="store_true", help="positions [16, 16 + K) only (kernel-trace runs)")
    args = ap.parse_args()
    args.batches = [int(b) for b in args.batches.split(",") if b]
    with torch.no_grad():
        if args.attn or args.attn_only:
            bench_attention(args)
        if not args.attn_only:
            bench_steps(args)


if __name__ == "__main__":
    main()
