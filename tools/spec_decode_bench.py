"""Speculative greedy decode (LlamaDecoder.generate_speculative) against the captured decode step, in one process
per run, on random-init E8P12 decoders of three shapes:

    7b          Llama-2-7B's shape on the persistent one-launch token
    7b-stagewise  the same with QUIP_BLOCK_ENGINE=0 (the stage-wise step)
    13b         Llama-2-13B's shape (hidden 5120: no persistent instantiation)

Per shape, two measurements:

  pass   the captured pass of k + 1 rows at k = 1, 2, 4, 7 and the captured step(), replayed ALTERNATELY (--rounds rounds of
         --steps replays each behind --warmup, device events), from position 16.  Reported: ms per replay of every round,
         medians, spreads, and the break-even mean acceptance per pass, pass_ms / step_ms - 1: a pass emits 1 + accepted
         tokens, so it pays once the mean number of accepted guesses per pass exceeds that.
  e2e    tokens/s of generate_speculative(128 tokens) with `prediction` set to the call's true continuation corrupted at rates
         0, 1/8, 1/4, 1/2 (every 8th / 4th / 2nd token replaced) -- that controls the acceptance on a random-init model --
         beside generate(128 tokens) on the captured step, alternating, host clock around a device synchronise, --reps times.
         The true continuation is the speculative route's own at the same k (ngram (0, 0): no guesses), since the chunk
         launches and the step's launches may break a near tie differently.  Every e2e line says whether the call returned
         that continuation (`same_tokens`: the guesses must never change the tokens).

One JSON line per measurement; --out also writes them to a file (profiles/spec_decode_bench.txt is such a file).

    python tools/spec_decode_bench.py [--shapes 7b,7b-stagewise,13b] [--steps 32] [--warmup 4] [--rounds 5] [--reps 3]
                                      [--layers N] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KS = (1, 2, 4, 7)
NGRAM = (1, 3)
RATES = ((0, "0"), (8, "1/8"), (4, "1/4"), (2, "1/2"))      # every n-th token replaced
N_TOKENS = 128
P0 = 16


def _events(run, steps, warmup, reset):
    reset()
    for _ in range(warmup):
        run()
    reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def _corrupt(truth, every, vocab):
    if not every:
        return truth.clone()
    at = torch.arange(truth.numel(), device=truth.device) % every == every - 1
    return torch.where(at, (truth + 1) % vocab, truth)


def bench_shape(name, D, args, emit):
    shapes = {"7b": (D.LLAMA2_7B, "1"), "7b-stagewise": (D.LLAMA2_7B, "0"),
              "13b": (D.LlamaShape(hidden=5120, ffn=13824, layers=40, heads=40, kv_heads=40), "1")}
    shape, engine = shapes[name]
    if args.layers:
        shape = D.LlamaShape(**{**shape.__dict__, "layers": args.layers})
    os.environ["QUIP_BLOCK_ENGINE"] = engine
    dec = D.LlamaDecoder(shape, "E8P12", max_len=512, device="cuda:0", seed=0, device_init=True)
    S = dec._spec_state()
    g = torch.Generator().manual_seed(1)
    prompt = torch.randint(0, shape.vocab, (P0 + 1,), generator=g).to("cuda:0")
    emit(dict(shape=name, hidden=shape.hidden, ffn=shape.ffn, layers=shape.layers, heads=shape.heads, vocab=shape.vocab,
              codebook="E8P12", block_eng=bool(dec.block_eng), token_tail=bool(dec._token_tail_on()), chain=bool(dec.chain),
              fused_prologue=bool(dec.fused_prologue), device=torch.cuda.get_device_name(0)))

    # ---- the captured pass against the captured step -------------------------------------------------------------------
    first = dec.generate(8, prompt=prompt).tolist()                      # captures the step
    emit(dict(shape=name, first_tokens=first))                           # (which model this is: device-side random init)
    for k in KS:
        dec.generate_speculative(4, prompt, k=k, ngram=NGRAM)            # captures the pass of k + 1 rows
    cands = {"step": dec.graph.replay}
    cands.update({f"pass_k{k}": dec._spec_graphs[(k, *NGRAM, None)].replay for k in KS})

    def reset():
        dec.pos.fill_(P0)
        for t in (S["rows"], S["n_draft"], S["out_len"], S["stats"]):
            t.zero_()
    ms = {c: [] for c in cands}
    for _ in range(args.rounds):
        for c, run in cands.items():                                     # alternating: every candidate sees the same machine
            ms[c].append(_events(run, args.steps, args.warmup, reset))
    status = int(S["stats"][3])
    med = {c: statistics.median(v) for c, v in ms.items()}
    emit(dict(shape=name, measure="pass", positions_from=P0, rounds=args.rounds, replays_per_round=args.steps, status=status,
              ms={c: [round(x, 4) for x in v] for c, v in ms.items()}, median_ms={c: round(v, 4) for c, v in med.items()},
              spread_us={c: round(1e3 * (max(v) - min(v)), 1) for c, v in ms.items()},
              break_even_accepted_per_pass={c: round(med[c] / med["step"] - 1, 3) for c in cands if c != "step"}))

    # ---- end to end ----------------------------------------------------------------------------------------------------
    runs, truths = {"generate": lambda: dec.generate(N_TOKENS, prompt=prompt)}, {}
    for k in KS:
        # (per k: the projections pick their kernel by the row count, and a near tie may fall the other way)
        truth = dec.generate_speculative(N_TOKENS + k + 1, prompt, k=k, ngram=(0, 0), use_graph=False).clone()
        for every, label in RATES:
            pred = _corrupt(truth, every, shape.vocab)
            runs[f"k{k}_corrupt_{label}"] = (lambda k=k, pred=pred: dec.generate_speculative(N_TOKENS, prompt, k=k, ngram=NGRAM,
                                                                                             prediction=pred))
            truths[f"k{k}_corrupt_{label}"] = truth[:N_TOKENS]
    secs, stats, result = {c: [] for c in runs}, {}, [None]
    for _ in range(args.reps):
        for c, fn in runs.items():
            secs[c].append(_wall(lambda: result.__setitem__(0, fn())))
            if c != "generate":
                # (the guesses must not change the tokens: the call returns the undrafted call's, whatever the prediction)
                stats[c] = dict(dec.spec_stats, same_tokens=bool(torch.equal(result[0], truths[c])))
    for c in runs:
        med_s = statistics.median(secs[c])
        rec = dict(shape=name, measure="e2e", run=c, n_tokens=N_TOKENS, reps=args.reps, seconds=[round(x, 4) for x in secs[c]],
                   tokens_per_s=round(N_TOKENS / med_s, 1),
                   vs_generate=round(statistics.median(secs["generate"]) / med_s, 3))
        if c in stats:
            st = stats[c]
            rec.update(passes=st["passes"], drafted=st["drafted"], accepted=st["accepted"],
                       accepted_per_pass=round(st["accepted"] / st["passes"], 3), same_tokens=st["same_tokens"])
        emit(rec)
    del dec, S, cands, runs
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="7b,7b-stagewise,13b")
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=0, help="override the number of blocks (rehearsals)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("spec_decode_bench: needs a GPU (there is no CPU path to time)")
    if P0 + (args.steps + args.warmup) * (max(KS) + 1) + max(KS) + 1 > 512:
        raise SystemExit("spec_decode_bench: --steps + --warmup too large for max_len 512")
    from quip_for_all_amd import decode as D
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    with torch.no_grad():
        for name in args.shapes.split(","):
            bench_shape(name, D, args, emit)
    if out:
        out.close()


if __name__ == "__main__":
    main()
