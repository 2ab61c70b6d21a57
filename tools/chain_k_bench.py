"""Captured bs=1 decode step of a Llama-shaped decoder of any shape on the stage-wise step: launches per block, tokens per
second and microseconds per block -- the figures DESIGN section 9 quotes for the shapes no persistent launch is compiled
for (Llama-2-13B: hidden 5120 = 5 x 1024, Qwen2-7B: 3584 = 7 x 512).

usage: python tools/chain_k_bench.py --hidden 5120 --ffn 13824 --layers 40 --heads 40 --kv-heads 40
           [--codebook E8P12] [--steps 64] [--warmup 16] [--runs 5] [--no-chain] [--json]

--no-chain builds the decoder with QUIP_CHAIN=0: the plain step, three launches per module.  Timing is the captured
step after `--warmup` replays (an idle device ramps its clocks over the first replays); every run
is `--steps` replays between two synchronisations; the median and the spread (max - min) of `--runs` runs are printed.
Launches per block are the quip_lib ops of one eager step (one launch each), see count_launches."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def count_launches(dec):
    """launches per block of the stage-wise step: every launch inside a block is one quip_lib op (a grouped op is one
    launch; out_transform_group issues one op per launch), so the quip_lib ops dispatched during one eager step are
    counted; the token's head (embedding, RMSNorm, lm_head product, arg-max) is not.  A kernel trace (rocprofv3
    --kernel-trace --stats) shows the same number."""
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode

    class Count(TorchDispatchMode):
        def __init__(self):
            super().__init__()
            self.block = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = func.name() if hasattr(func, "name") else str(func)
            if name.startswith("quip_lib::") and "argmax_step" not in name:
                self.block += 1
            return func(*args, **(kwargs or {}))

    dec.reset(1)
    with torch.no_grad():
        dec.step()                                   # warm: workspaces, lazily built tables
        c = Count()
        with c:
            dec.step()
    torch.cuda.synchronize()
    return c.block / len(dec.layers)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--hidden", type=int, default=5120)
    ap.add_argument("--ffn", type=int, default=13824)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--heads", type=int, default=40)
    ap.add_argument("--kv-heads", type=int, default=None)
    ap.add_argument("--codebook", default="E8P12")
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=16)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-len", type=int, default=256)
    ap.add_argument("--no-chain", action="store_true", help="QUIP_CHAIN=0: the plain step")
    ap.add_argument("--no-launch-count", action="store_true", help="skip the counting step")
    ap.add_argument("--json", action="store_true", help="one JSON line instead of text")
    a = ap.parse_args()
    if a.no_chain:
        os.environ["QUIP_CHAIN"] = "0"
    import torch
    from quip_for_all_amd import decode as D
    kvh = a.kv_heads if a.kv_heads is not None else a.heads
    shape = D.LlamaShape(hidden=a.hidden, ffn=a.ffn, layers=a.layers, heads=a.heads, kv_heads=kvh)
    dec = D.LlamaDecoder(shape, a.codebook, max_len=a.max_len, device="cuda:0", seed=0, device_init=True)
    flags = {k: bool(getattr(dec, k, False)) for k in ("chain", "fused_prologue", "attn_z", "qkv_fused", "o_fused", "ffn_eng",
                                                       "block_eng")}
    per_block = None if a.no_launch_count else count_launches(dec)
    dec.graph = None
    dec.reset(1)
    dec.capture()
    for _ in range(a.warmup):
        dec.graph.replay()
    times = []
    for _ in range(a.runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            dec.graph.replay()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) / a.steps)
    toks = sorted(1.0 / t for t in times)
    med = statistics.median(times)
    codes = a.layers * (2 * a.hidden * a.hidden + 2 * a.hidden * (a.hidden // a.heads) * kvh + 3 * a.hidden * a.ffn) // 4
    res = {
        "hidden": a.hidden, "ffn": a.ffn, "layers": a.layers, "heads": a.heads, "kv_heads": kvh, "codebook": a.codebook,
        **flags,
        "launches_per_block": None if per_block is None else round(per_block, 2),
        "tok_s_median": round(1.0 / med, 2), "tok_s_min": round(toks[0], 2), "tok_s_max": round(toks[-1], 2),
        "tok_s_spread": round(toks[-1] - toks[0], 2),
        "us_per_block": round(med * 1e6 / a.layers, 2), "ms_per_token": round(med * 1e3, 4),
        "hbm_fraction_of_8TBs": round(codes / med / 8e12, 4), "runs": a.runs, "steps": a.steps, "warmup": a.warmup,
    }
    if a.json:
        print(json.dumps(res))
        return
    print(" ".join(f"{k}={v}" for k, v in flags.items()))
    print(f"hidden {a.hidden} ffn {a.ffn} x {a.layers} {a.codebook}: launches per block {res['launches_per_block']}; "
          f"{res['tok_s_median']:.2f} tok/s (median of {a.runs}, spread {res['tok_s_spread']:.2f}: "
          f"{res['tok_s_min']:.2f} .. {res['tok_s_max']:.2f}); {res['us_per_block']:.1f} us per block incl. head; "
          f"{res['hbm_fraction_of_8TBs']:.3f} of 8 TB/s")


if __name__ == "__main__":
    main()
