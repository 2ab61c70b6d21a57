"""What LoRA adapters cost on the decoders: a Llama-2-7B-shaped random decoder (E8P12, `enable_lora(4, 16)`), captured steps,
the variants replayed alternately in one process, device events, medians of `--rounds` rounds with their spreads.

bs = 1, on both routes (`_block`: the stage-wise step; `_step_fused`: chain launches / GEMV prologues, `lora_fused_step`):
the step with no adapter launches (nothing loaded), r = 16 on q, v and r = 16 on all seven.  B = 16: no adapter launches
against four adapters mixed over the slots (and the same captured step with no slot selecting one).  Then both launches
alone at the 7B shapes, 1 and 16 rows.  A captured step keeps its launch list, so the variants are captured in the order
the adapters are loaded; the index tensors are set before each timing.

    python tools/lora_bench.py [--steps 64] [--warmup 8] [--rounds 5] [--batch 16] [--layers 32] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEFT = {"q": "self_attn.q_proj", "k": "self_attn.k_proj", "v": "self_attn.v_proj", "o": "self_attn.o_proj",
        "gate": "mlp.gate_proj", "up": "mlp.up_proj", "down": "mlp.down_proj"}
ALL = tuple(PEFT)


def _adapter(dims, layers, r, targets, seed):
    g = torch.Generator().manual_seed(seed)
    t = {}
    for i in range(layers):
        for m in targets:
            n_in, n_out = dims[m]
            t[f"base_model.model.model.layers.{i}.{PEFT[m]}.lora_A.weight"] = \
                (0.2 * torch.randn(r, n_in, generator=g) / n_in ** 0.5).half()
            t[f"base_model.model.model.layers.{i}.{PEFT[m]}.lora_B.weight"] = (0.2 * torch.randn(n_out, r, generator=g)).half()
    cfg = {"peft_type": "LORA", "r": r, "lora_alpha": 2 * r, "target_modules": [PEFT[m].split(".")[1] for m in targets]}
    return t, cfg


def _time(replay, steps, warmup, reset):
    reset()
    for _ in range(warmup):
        replay()
    reset()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def _alternate(what, variants, args, emit, extra=None):
    """variants: name -> (replay, reset); every round times each variant once, in order"""
    ms = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, (replay, reset) in variants.items():
            ms[n].append(_time(replay, args.steps, args.warmup, reset))
    rec = dict(step=what, rounds=args.rounds, steps_per_round=args.steps)
    for n, v in ms.items():
        rec[n] = dict(ms=[round(x, 4) for x in v], median_ms=round(statistics.median(v), 4),
                      spread_us=round(1e3 * (max(v) - min(v)), 2))
    rec.update(extra or {})
    emit(rec)
    return {n: (statistics.median(v), max(v) - min(v)) for n, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--pos", type=int, default=16)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_bench: needs a GPU (there is no CPU path to time)")
    from quip_for_all_amd import decode as D
    out = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()
    shape = D.LlamaShape(layers=args.layers)
    kv = shape.kv_heads * shape.head_dim
    dims = {"q": (shape.hidden, shape.q_width), "k": (shape.hidden, kv), "v": (shape.hidden, kv),
            "o": (shape.q_width, shape.hidden), "gate": (shape.hidden, shape.ffn), "up": (shape.hidden, shape.ffn),
            "down": (shape.ffn, shape.hidden)}
    max_len = args.pos + args.steps + args.warmup + 16
    dev = "cuda:0"
    with torch.no_grad():
        dec = D.LlamaDecoder(shape, "E8P12", max_len=max_len, device=dev, seed=0, device_init=True)
        before = dict(fused_prologue=bool(dec.fused_prologue), chain=bool(dec.chain), ffn_eng=bool(dec.ffn_eng),
                      block_eng=bool(dec.block_eng), attn_z=bool(dec.attn_z))
        dec.enable_lora(max_adapters=4, max_rank=16)
        emit(dict(model="Llama-2-7B-shaped random init", hidden=shape.hidden, ffn=shape.ffn, layers=shape.layers,
                  heads=shape.heads, kv_heads=shape.kv_heads, vocab=shape.vocab, codebook="E8P12", max_len=max_len,
                  before_enable_lora=before, fused_prologue=bool(dec.fused_prologue), chain=bool(dec.chain),
                  adapter_slot_mb=round(dec.lora.bytes_per_slot() / 2 ** 20, 2), device=torch.cuda.get_device_name(0)))
        B = args.batch
        bd = dec.batched(B)
        g = torch.Generator(device=dev).manual_seed(1)
        bs1, b16 = {}, {}

        def capture_bs1(tag, adapter):
            for route, fused in (("block", False), ("fused", True)):
                dec.lora_fused_step, dec.graph = fused, None
                dec.set_adapter(adapter)
                dec.capture()
                graph, idx = dec.graph, dec.lora.index(adapter)

                def reset(idx=idx):
                    dec.lora.idx.fill_(idx)
                    dec.pos.fill_(args.pos)
                bs1[f"{tag}_{route}"] = (graph.replay, reset)
            dec.lora_fused_step, dec.graph = True, None

        def capture_b16(tag, slots):
            bd.graph = None
            bd.capture()
            graph = bd.graph
            idx = torch.tensor(slots, dtype=torch.int32, device=dev)

            def reset():
                bd.slot_adapter.copy_(idx)
                bd.pos.fill_(args.pos)
                bd.tok.copy_(torch.randint(0, shape.vocab, (B,), generator=g, device=dev))
            b16[tag] = (graph.replay, reset)
        capture_bs1("none", None)                       # nothing loaded: no adapter launch in the step
        capture_b16("none", [-1] * B)
        dec.load_adapter("qv16", *_adapter(dims, shape.layers, 16, ("q", "v"), 1))
        capture_bs1("qv16", "qv16")
        for j in (1, 2, 3):
            dec.load_adapter(f"all16_{j}", *_adapter(dims, shape.layers, 16, ALL, 1 + j))
        capture_bs1("all16", "all16_1")
        capture_b16("mixed4", [b % 4 for b in range(B)])
        lora_graph_reset = b16["mixed4"][1]

        def reset_idle():
            lora_graph_reset()
            bd.slot_adapter.fill_(-1)
        b16["mixed4_graph_no_slot_selected"] = (b16["mixed4"][0], reset_idle)
        med = _alternate("bs1", bs1, args, emit)
        # the default bs = 1 route with adapters: _step_fused only if faster by more than twice the larger spread
        for tag in ("qv16", "all16"):
            (mb, sb), (mf, sf) = med[f"{tag}_block"], med[f"{tag}_fused"]
            emit(dict(decision=tag, block_minus_fused_us=round(1e3 * (mb - mf), 2), bar_us=round(2e3 * max(sb, sf), 2),
                      fused_is_faster=bool(mb - mf > 2 * max(sb, sf))))
        _alternate(f"B{B}", b16, args, emit, {"batch": B, "regimes": bd.regimes()})
        # both launches alone at the 7B shapes
        L0 = dec.layers[0]
        lay = L0["lora"]
        for rows in (1, B):
            idx = torch.tensor([b % 4 for b in range(rows)], dtype=torch.int32, device=dev)
            x = torch.randn(rows, shape.hidden, device=dev).half()
            u, gt = torch.randn(rows, shape.ffn, device=dev).half(), torch.randn(rows, shape.ffn, device=dev).half()
            ys = {m: torch.randn(rows, dims[m][1], device=dev).half() for m in ALL}
            ts = {grp: torch.randn(rows, A.shape[1], device=dev) for grp, A in lay.A.items()}
            kernels = {
                "shrink_qkv_norm_in4096_R48": lambda: lay.shrink("qkv", x, idx, rms_weight=L0["ln1"], rms_eps=shape.rms_eps),
                "shrink_o_in4096_R16": lambda: lay.shrink("o", x, idx),
                "shrink_gu_norm_in4096_R32": lambda: lay.shrink("gu", x, idx, rms_weight=L0["ln2"], rms_eps=shape.rms_eps),
                "shrink_down_gate_in11008_R16": lambda: lay.shrink("down", u, idx, gate=gt),
                "expand_qkv_3x4096": lambda: lay.expand("qkv", ts["qkv"], [ys["q"], ys["k"], ys["v"]], idx),
                "expand_o_4096": lambda: lay.expand("o", ts["o"], [ys["o"]], idx),
                "expand_gu_2x11008": lambda: lay.expand("gu", ts["gu"], [ys["gate"], ys["up"]], idx),
                "expand_down_4096": lambda: lay.expand("down", ts["down"], [ys["down"]], idx),
            }
            rec = dict(kernels_alone_rows=rows, launches_per_replay=20, replays_per_round=20, rounds=args.rounds)
            for name, fn in kernels.items():
                # 20 launches back to back in one captured graph: the device's time per launch, not the host's
                graph, _ = D.capture_graph(fn, lambda fn=fn: [fn() for _ in range(20)] and None)
                us = [1e3 * _time(graph.replay, 20, 3, lambda: None) / 20 for _ in range(args.rounds)]
                rec[name] = dict(median_us=round(statistics.median(us), 2), spread_us=round(max(us) - min(us), 2))
            emit(rec)
    if out:
        out.close()


if __name__ == "__main__":
    main()
