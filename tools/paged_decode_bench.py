"""The paged batch decoder against the contiguous one on the 7B-shaped random decoder (E8P12), B = 16, captured steps.

Both decoders live in one process on the same modules.  After warm-up replays of both, --rounds rounds alternate them:
per round --steps replays of each from the same start position, timed with device events; short context (positions from
16) and --long-pos.  The figure to read is the paged / contiguous ratio of the medians next to the spread of the rounds
(min .. max of each): a difference inside that spread is not a difference.  Then the attention launch alone, both ways,
through captured graphs, at --long-pos: same bytes streamed, the paged one through a shuffled block table.

One JSON line per measurement on stdout; --out also writes them, with a header, to a profile file.

    python tools/paged_decode_bench.py [--steps 48] [--rounds 5] [--long-pos 2048] [--out profiles/paged_decode_bench.txt]"""
import argparse
import json
import os
import random
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = 16


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


def _alternate(name, contiguous, paged, args):
    """contiguous / paged: (graph, reset) -> one result line"""
    for graph, reset in (contiguous, paged):
        reset()
        _replays(graph, args.warmup)
    ms = {"contiguous": [], "paged": []}
    for _ in range(args.rounds):
        for key, (graph, reset) in (("contiguous", contiguous), ("paged", paged)):
            reset()
            ms[key].append(_replays(graph, args.steps))
    res = {"what": name, "unit": "ms per replay", "rounds": args.rounds, "replays_per_round": args.steps,
           "contiguous": _summary(ms["contiguous"]), "paged": _summary(ms["paged"])}
    res["paged_over_contiguous"] = round(res["paged"]["median"] / res["contiguous"]["median"], 4)
    res["spread_contiguous"] = round(res["contiguous"]["max"] / res["contiguous"]["min"] - 1, 4)
    res["spread_paged"] = round(res["paged"]["max"] / res["paged"]["min"] - 1, 4)
    return res


def bench_steps(args, emit):
    from quip_for_all_amd import decode as D
    max_len = args.long_pos + args.steps + args.warmup + 16
    dec = D.LlamaDecoder(D.LLAMA2_7B, "E8P12", max_len=max_len, device="cuda:0", seed=0, device_init=True)
    ref, pg = dec.batched(B), dec.batched(B, paged=True)
    ref.capture()
    pg.capture()
    # every slot holds all its pages, handed out in a shuffled order: the step reads a scattered cache
    ids = list(range(pg.n_pages))
    random.Random(0).shuffle(ids)
    pg.pool.free = ids
    for b in range(B):
        pg.pool.reserve(b, max_len)
    pg._push_table()
    tok = torch.randint(0, dec.s.vocab, (B,), generator=torch.Generator().manual_seed(1)).to("cuda:0")
    emit({"what": "setup", "batch": B, "max_len": max_len, "pages": pg.n_pages, "page_MB_all_layers":
          round(2 * dec.s.layers * dec.s.kv_heads * 64 * dec.s.head_dim * 2 / 2 ** 20, 1), "regimes": ref.regimes()})
    for name, p0 in (("step_short", 16), ("step_long", args.long_pos)):
        def reset(d):
            d.pos.fill_(p0)
            d.tok.copy_(tok)
        r = _alternate(name, (ref.graph, lambda: reset(ref)), (pg.graph, lambda: reset(pg)), args)
        r["positions"] = [p0, p0 + args.steps]
        for k in ("contiguous", "paged"):
            r[f"tok_s_{k}"] = round(B * 1e3 / r[k]["median"], 1)
        emit(r)
    del ref, pg, dec
    torch.cuda.empty_cache()


def bench_attention(args, emit):
    import quip_for_all_amd  # noqa: F401
    import quip_for_all_amd.paged_attn  # noqa: F401
    from quip_for_all_amd.batch_decode import rope_attn_batched_workspace
    heads, kvh, hd, P, dev = 32, 32, 128, args.long_pos, "cuda:0"
    max_pages = P // 64 + 1
    max_len = max_pages * 64
    kc = torch.randn(B, kvh, max_len, hd, device=dev).half()
    vc = torch.randn_like(kc)
    ids = list(range(B * max_pages))
    random.Random(0).shuffle(ids)
    table = torch.tensor(ids, dtype=torch.int32, device=dev).view(B, max_pages)
    kpool, vpool = torch.randn(B * max_pages, kvh, 64, hd, device=dev).half(), torch.randn(B * max_pages, kvh, 64, hd, device=dev).half()
    q = torch.randn(B, heads, hd, device=dev).half()
    k, v = torch.randn(B, kvh, hd, device=dev).half(), torch.randn(B, kvh, hd, device=dev).half()
    cos, sin = torch.randn(max_len, hd, device=dev), torch.randn(max_len, hd, device=dev)
    pos = torch.full((B,), P, dtype=torch.long, device=dev)
    ws = [rope_attn_batched_workspace(B, heads, hd, dev) for _ in range(2)]
    graphs = []
    for fn in (lambda: torch.ops.quip_lib.rope_attn_decode_batched(q, k, v, cos, sin, pos, kc, vc, ws[0], 0),
               lambda: torch.ops.quip_lib.rope_attn_decode_paged(q, k, v, cos, sin, pos, table, kpool, vpool, ws[1], 0)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(args.attn_launches):
                fn()
        graphs.append(g)
    r = _alternate("attention_launch_alone", (graphs[0], lambda: None), (graphs[1], lambda: None), args)
    nbytes = B * 2 * kvh * (P + 1) * hd * 2
    r.update({"shape": f"B={B} heads={heads} kv_heads={kvh} hd={hd} positions={P + 1}", "launches_per_replay": args.attn_launches,
              "cache_bytes_per_launch": nbytes})
    for key in ("contiguous", "paged"):
        us = r[key]["median"] * 1e3 / args.attn_launches
        r[f"us_per_launch_{key}"] = round(us, 2)
        r[f"cache_TBps_{key}"] = round(nbytes / (us * 1e-6) / 1e12, 3)
    emit(r)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--long-pos", type=int, default=2048)
    ap.add_argument("--attn-launches", type=int, default=32, help="attention launches per captured graph")
    ap.add_argument("--attn-only", action="store_true")
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("paged_decode_bench: needs a GPU (nothing is measured without one)")
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    with torch.no_grad():
        if not args.attn_only:
            bench_steps(args, emit)
        bench_attention(args, emit)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# tools/paged_decode_bench.py: paged against contiguous batched decode, 7B shape, E8P12, B = 16, captured\n"
                    "# steps, device events; contiguous and paged alternate round by round in one process after warm-up replays.\n"
                    "# spread_* = max / min - 1 over the rounds of one side: a paged_over_contiguous inside it is no difference.\n"
                    f"# device: {torch.cuda.get_device_name(0)}; arguments: {vars(args)}\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
