#!/usr/bin/env python3
"""The grouped skinny launch (quip_lib::mm_skinny_group, csrc/e8p_skinny_group.hip) against the separate launches it
replaces, product ops alone: the q / k / v and gate / up groups of the 7B, Llama-3-8B and 70B blocks at M = 8, 16, 31.
Both sides are captured replays of NB different blocks' codes (more bytes than the L2 / MALL keep), timed alternately in
one process: ROUNDS rounds of [separate, grouped]; a side's figure is the median over the rounds of us per group, its
spread the max - min over the rounds.  The verdict column is the rule of skinny_group_supported: grouped wins when it is
faster by more than twice the larger spread.  usage: python tools/skinny_group_bench.py [rounds]"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quip_for_all_amd as Q  # noqa: E402

DEV = "cuda:0"
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
GROUPS = [("7B q/k/v", (4096, 4096, 4096), 4096), ("7B gate/up", (11008, 11008), 4096),
          ("8B q/k/v", (4096, 1024, 1024), 4096), ("8B gate/up", (14336, 14336), 4096),
          ("70B q/k/v", (8192, 1024, 1024), 8192), ("70B gate/up", (28672, 28672), 8192)]
CODEBOOKS = [("E8P12", torch.int16, GROUPS), ("E8P12RVQ4B", torch.int32, GROUPS[:2])]


def capture(fns):
    for f in fns:
        f()
    torch.cuda.synchronize()
    gr, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st), torch.cuda.graph(gr, stream=st):
        for f in fns:
            f()
    torch.cuda.synchronize()
    return gr


def replay_us(gr, per):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    gr.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def stats(ts):
    ts = sorted(ts)
    return ts[len(ts) // 2], ts[-1] - ts[0]


def main():
    assert torch.cuda.is_available(), "needs the GPU: no fall-back"
    gen = torch.Generator().manual_seed(0)
    print(f"# {torch.cuda.get_device_name(0)}, {ROUNDS} rounds of [separate, grouped] replays, us per group: median (spread)")
    for cbid, qdtype, groups in CODEBOOKS:
        cb = Q.codebook.codebook_id[cbid](inference=True).to(DEV)
        for name, ns, k in groups:
            nbytes = sum(ns) * (k // 8) * qdtype.itemsize
            nb = max(4, min(24, (600 << 20) // nbytes))          # blocks cycled per replay: about 600 MB of codes
            info = torch.iinfo(qdtype)
            blocks = [[torch.randint(info.min, info.max, (n, k // 8), dtype=torch.int64, generator=gen).to(qdtype).to(DEV)
                       for n in ns] for _ in range(nb)]
            for M in (8, 16, 31):
                xs = [torch.randn(M, k, generator=gen).half().to(DEV) for _ in ns]
                if not cb.skinny_group_supported(M, list(ns), k):
                    print(f"{cbid:11s} {name:12s} M={M:2d}: not a group the launch takes")
                    continue
                sep = capture([(lambda qs=qs: [cb.mm_skinny(x, q) for x, q in zip(xs, qs)]) for qs in blocks])
                grp = capture([(lambda qs=qs: cb.mm_skinny_group(xs, qs)) for qs in blocks])
                for qs in blocks[:1]:
                    assert all(torch.equal(a, cb.mm_skinny(x, q)) for a, x, q in zip(cb.mm_skinny_group(xs, qs), xs, qs))
                ts, tg = [], []
                for _ in range(ROUNDS):
                    ts.append(replay_us(sep, nb))
                    tg.append(replay_us(grp, nb))
                (ms, ss), (mg, sg) = stats(ts), stats(tg)
                verdict = "grouped wins" if ms - mg > 2 * max(ss, sg) else ("separate wins" if mg - ms > 2 * max(ss, sg)
                                                                            else "inside the spread")
                print(f"{cbid:11s} {name:12s} M={M:2d}: separate {ms:7.2f} ({ss:5.2f})  grouped {mg:7.2f} ({sg:5.2f})  "
                      f"{nbytes / mg / 1e6:5.2f} TB/s of codes grouped  -> {verdict}", flush=True)
                del sep, grp


if __name__ == "__main__":
    main()
