#!/usr/bin/env python
"""A Mixtral-shaped MoE MLP half (hidden 4096, ffn 14336, E = 8, top_k = 2; random init) at M in {1, 16} rows, graph-timed:
QuantMoeMlp.forward_rows (nine routed launches, csrc/e8p_skinny_moe.hip + moe_rows.hip.h) against the loop over the experts
on the modules' own forward (QuantMoeMlp._experts_loop; the ids are read by the host BEFORE the capture, so its graph holds
ONE routing: that of the input it was captured on).
Both graphs replay the same input; the two alternate in one process, `--rounds` rounds of `--reps` replays each, and the
median round and the spread are printed per variant.  --experts / --top-k / --rows change the shape (E = 64 at 31 rows is
the router's worst case: every workgroup routes all rows)."""
import argparse
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=4096)
    ap.add_argument("--ffn", type=int, default=14336)
    ap.add_argument("--experts", type=int, default=8)
    ap.add_argument("--top-k", type=int, default=2)
    ap.add_argument("--rows", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    from quip_for_all_amd import decode as D
    from quip_for_all_amd.moe import QuantMoeMlp
    dev, g = "cuda:0", torch.Generator().manual_seed(0)
    gq = torch.Generator(device=dev).manual_seed(0)
    ql = lambda i, o: D.random_quant_linear(i, o, "E8P12", gq, dev)  # noqa: E731
    triples = D.random_experts(ql, a.hidden, a.ffn, a.experts)
    router = (torch.randn(a.experts, a.hidden, generator=g) / 4).to(torch.float16)
    mlp = QuantMoeMlp(router, triples, a.top_k).to(dev).eval()
    ln = torch.ones(a.hidden, dtype=torch.float16, device=dev)
    for M in a.rows:
        h = torch.randn(M, a.hidden, generator=g).to(torch.float16).to(dev)
        graphs = {}
        with torch.no_grad():
            _, start, pair_of, weight = torch.ops.quip_lib.moe_route_rows(h, ln, mlp.router, None, None, a.top_k, 1, True, 1e-5)
            e_of = torch.repeat_interleave(torch.arange(a.experts, device=dev), start.diff().long())
            owned = [((pair_of[e_of == e] // a.top_k).long(), (pair_of[e_of == e] % a.top_k).long()) for e in range(a.experts)]
            w = torch.zeros(M * a.top_k, device=dev).index_put((pair_of.long(),), weight).view(M, a.top_k)
            for name, fn in (("routed", lambda: mlp.forward_rows(h, ln, 1e-5)),
                             ("expert loop", lambda: mlp._experts_loop(h, ln, 1e-5, w, owned))):
                graphs[name] = D.capture_graph(lambda fn=fn: (fn(), fn()), fn)[0]
        times = {name: [] for name in graphs}
        for _ in range(a.rounds):
            for name, graph in graphs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    graph.replay()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e3 / a.reps)
        print(f"M = {M}, E = {a.experts}, top_k = {a.top_k}, hidden {a.hidden}, ffn {a.ffn}: " + " | ".join(
            f"{name} {statistics.median(t):8.1f} us (min {min(t):.1f}, max {max(t):.1f})" for name, t in times.items()))


if __name__ == "__main__":
    main()
