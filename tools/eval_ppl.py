#!/usr/bin/env python3
"""Perplexity of a token file under a QuIP# checkpoint (or a random model of a given shape) with LlamaDecoder.perplexity:
the usual protocol, windows of --window tokens every --stride tokens, each scored from position 0, every target scored once.

  eval_ppl.py CHECKPOINT_DIR --tokens ids.npy [--window 2048] [--stride N] [--chunk 512]
  eval_ppl.py --shape LLAMA2_7B --codebook E8P12 --random-tokens 8192 --seed 0

  CHECKPOINT_DIR     a directory load_quantized_model reads (then LlamaDecoder.from_hf)
  --shape / --codebook   instead of a checkpoint: a random model of that shape (timing and plumbing, not quality)
  --tokens FILE      a .npy file of integer token ids, any shape, read in order (no dataset is fetched, nothing is tokenised)
  --random-tokens N --seed S   instead of a file: N uniform ids from seed S
Prints one JSON line: ppl, nll_sum, n_scored, argmax_hits, seconds, tokens_per_s, window, stride, chunk."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("checkpoint", nargs="?")
    ap.add_argument("--shape")
    ap.add_argument("--codebook", default="E8P12")
    ap.add_argument("--tokens")
    ap.add_argument("--random-tokens", type=int)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--stride", type=int)
    ap.add_argument("--chunk", type=int, default=512)
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args()
    if (a.checkpoint is None) == (a.shape is None):
        ap.error("give a checkpoint directory or --shape NAME, not both")
    if (a.tokens is None) == (a.random_tokens is None):
        ap.error("give --tokens FILE or --random-tokens N, not both")
    if a.checkpoint:
        from quip_for_all_amd import load_quantized_model
        model = load_quantized_model(a.checkpoint, device_map=a.device)
        dec = D.LlamaDecoder.from_hf(model, max_len=a.window, device=a.device)
    else:
        dec = D.LlamaDecoder(getattr(D, a.shape), a.codebook, max_len=a.window, device=a.device, seed=a.seed, device_init=True)
    if a.tokens:
        ids = np.load(a.tokens)
        if not np.issubdtype(ids.dtype, np.integer):
            raise SystemExit(f"{a.tokens}: {ids.dtype} is not an integer type")
        toks = torch.from_numpy(ids.astype(np.int64).reshape(-1))
    else:
        toks = torch.randint(0, dec.s.vocab, (a.random_tokens,), generator=torch.Generator().manual_seed(a.seed))
    if int(toks.min()) < 0 or int(toks.max()) >= dec.s.vocab:
        raise SystemExit(f"token ids outside [0, {dec.s.vocab})")
    toks = toks.to(a.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = dec.perplexity(toks, window=a.window, stride=a.stride, chunk=a.chunk)      # (ends in a read of the totals)
    secs = time.perf_counter() - t0
    res.update(seconds=round(secs, 4), tokens_per_s=round(toks.numel() / secs, 1), window=a.window,
               stride=a.window if a.stride is None else a.stride, chunk=a.chunk)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
