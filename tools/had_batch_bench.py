#!/usr/bin/env python3
"""Prefill-sized Hadamard launches (rows = 16 x 2048): time and achieved HBM rate (read + write) per transform.
With a trailing `mix`: the group launch's route (the switch QUIP_HAD_MIX_BATCH unset) beside had_transform_mix_batch on the
same operands, alternating in one process: median and spread (max - min) of ROUNDS rounds of 10 launches each."""
import math, os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import quip_for_all_amd  # noqa
from quip_for_all_amd.quant import get_hadK
dev = "cuda"
rows = int(sys.argv[1]) if len(sys.argv) > 1 else 32768
def t(fn, n=10):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n): fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / n
op = torch.ops.quip_lib
RAND = not (len(sys.argv) > 3 and sys.argv[3] == 'tables')   # 'tables': get_hadK(use_rand=False) factors
sizes = [int(v) for v in sys.argv[2].split(',')] if len(sys.argv) > 2 else [4096, 11008, 1024, 8192]
MIX = sys.argv[-1] == 'mix'
ROUNDS = 7
def ab(old, new):
    """[(median, spread)] of the two routes, a round of each in turn"""
    ts = ([], [])
    for _ in range(ROUNDS):
        ts[0].append(t(old)); ts[1].append(t(new))
    return [(sorted(v)[ROUNDS // 2], max(v) - min(v)) for v in ts]
for n in sizes:
    had, K, qn = get_hadK(n, RAND)
    if qn != n: continue
    if MIX:
        hd = had.to(dev).half().contiguous()
        x = torch.randn(rows, n, device=dev).half(); su = torch.ones(n, device=dev).half(); s = 1.0 / math.sqrt(n // K)
        gb = 2 * rows * n * 2 / 1e9
        for side, tr, pre, post in (("input side", True, su, None), ("output side", False, None, su)):
            (to, so), (tn, sn) = ab(lambda: op.had_transform_fused(x, n, n, K, hd, tr, pre, None, post, None, s, None, None, 1e-5, None),
                                    lambda: op.had_transform_mix_batch(x, n, n, K, hd, tr, pre, None, post, None, s))
            print(f"n={n:6d} K={K:3d} rows={rows} {side:11s}: switch off {to:.3f} ms +- {so:.3f} ({gb / to:.2f} TB/s r+w)   mix_batch "
                  f"{tn:.3f} ms +- {sn:.3f} ({gb / tn:.2f} TB/s r+w)   {'beats' if to - tn > 2 * max(so, sn) else 'DOES NOT beat'} "
                  f"it by more than twice the larger spread", flush=True)
        del x
        continue
    hd = None if had is None else had.to(dev).half().contiguous()
    x = torch.randn(rows, n, device=dev).half(); su = torch.ones(n, device=dev).half()
    ti = t(lambda: op.had_transform_fused(x, n, n, K, hd, True, su, None, None, None, 1.0 / math.sqrt(n // K), None, None, 1e-5, None))
    to = t(lambda: op.had_transform_fused(x, n, n, K, hd, False, None, None, su, None, 1.0, None, None, 1e-5, None))
    gb = 2 * rows * n * 2 / 1e9
    print(f"n={n:6d} K={K:3d} rows={rows}: input side {ti:.3f} ms ({gb / ti:.2f} TB/s r+w)  output side {to:.3f} ms ({gb / to:.2f} TB/s r+w)", flush=True)
    del x
y = torch.empty(rows, 4096, device=dev).half(); z = torch.randn(rows, 4096, device=dev).half()
tc = t(lambda: y.copy_(z))
print(f"torch copy_ of {rows} x 4096 fp16: {tc:.3f} ms ({2 * rows * 4096 * 2 / 1e9 / tc:.2f} TB/s r+w)")
