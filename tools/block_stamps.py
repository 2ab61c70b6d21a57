#!/usr/bin/env python3
"""Phase clocks of one block inside the persistent token launch (csrc/decode_block.hip, BSTAMP), Llama-2-7B shape.
usage: python tools/block_stamps.py [layers] [dbg_layer] [pos] [g8]      (g8: the Llama-3-8B shape, decode_block_g8.hip)
       python tools/block_stamps.py [layers] tail [pos] [g8]           the token's tail behind the last block (csrc/token_tail.hip.h:
                                                                       dbg_layer = layers reuses the slots; the device-wide 100 MHz clock)
QUIP_MLP_STAMPS=1 with a library built with -DQUIP_MLP_STAMPS=1 (tools/dbg/build_variant.sh, QUIP_LIB_PATH): the finer stamps inside
the MLP edge (gate / up products, row owners, K-mix and planes) instead of those inside the two 4096-wide edges.
QUIP_WAIT_STAMPS=1 with a library built with -DQUIP_WAIT_STAMPS=1: the stamps around the waits of the four product phases (q / k / v,
o, gate / up, down); QUIP_WAIT_STAMPS=2 (-DQUIP_WAIT_STAMPS=2): one stamp per wave in front of the barrier behind the K-mix.  A stamp
is a store that the next wait for the whole queue waits for: take the phase totals from an unstamped library."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quip_for_all_amd import decode as D  # noqa: E402

layers = int(sys.argv[1]) if len(sys.argv) > 1 else 32
tail = len(sys.argv) > 2 and sys.argv[2] == "tail"
dl = layers if tail else (int(sys.argv[2]) if len(sys.argv) > 2 else layers // 2)
pos0 = int(sys.argv[3]) if len(sys.argv) > 3 else 100
g8 = len(sys.argv) > 4 and sys.argv[4] == "g8"
shape = (D.LlamaShape(hidden=4096, ffn=14336, layers=layers, heads=32, kv_heads=8, vocab=32000) if g8 else
         D.LlamaShape(hidden=4096, ffn=11008, layers=layers, heads=32, kv_heads=32, vocab=32000))
dec = D.LlamaDecoder(shape, "E8P12", max_len=max(256, pos0 + 16), device="cuda:0", seed=0, device_init=True)
assert dec.block_eng
dec.reset(7)
dec.pos.fill_(pos0)
h = dec.embed[dec.tok].reshape(-1)
dbg = torch.zeros(256 * 32, dtype=torch.int64, device="cuda:0")
if tail:
    # stamps of the whole-token launch: 0 tail entered, 1 x in registers (final norm), 2 rows streamed, 3 granule published,
    # 4 (workgroup 0) token and position stored
    logits = torch.empty(1, shape.vocab, dtype=torch.float16, device="cuda:0")
    runs = []
    for it in range(8):
        dbg.zero_()
        dec.tok.fill_(7)
        dec.pos.fill_(pos0)
        torch.ops.quip_lib.block_engine_token(dec.eng_layers, dec.tok, dec.pos, dec.embed, dec.final_norm, dec.lm_head, logits,
                                              dec.cos, dec.sin, dec.eng_grid, dec.eng_ws, layers, dec.max_len, shape.rms_eps,
                                              1.0 / math.sqrt(128), dbg, dl | 0x10000, dec.eng_codebook, 0.0, dec.eng_shape)
        torch.cuda.synchronize()
        if it >= 2:
            runs.append(dbg.cpu().numpy().reshape(256, 32)[:, :5].astype(np.float64) / 100.0)      # us
    T = np.stack(runs)                          # (runs, 256, 5)
    t0 = T[:, :, 0].min(axis=1, keepdims=True)
    print(f"status {dec.engine_status()}; the token's tail behind block {layers - 1}, us (median over {len(runs)} launches; 100 MHz device clock):")
    print(f"  workgroups enter the tail over            {np.median(T[:, :, 0].max(axis=1) - t0[:, 0]):7.2f}")
    print(f"  final norm, x in registers (per wg, mean) {np.median((T[:, :, 1] - T[:, :, 0]).mean(axis=1)):7.2f}")
    print(f"  lm_head rows (per wg, mean | slowest)     {np.median((T[:, :, 2] - T[:, :, 1]).mean(axis=1)):7.2f} | {np.median((T[:, :, 2] - T[:, :, 1]).max(axis=1)):7.2f}")
    print(f"  first entry -> last workgroup streamed    {np.median(T[:, :, 2].max(axis=1) - t0[:, 0]):7.2f}   ({shape.vocab * 8192 / 1e6:.0f} MB: "
          f"{shape.vocab * 8192 / 1e6 / np.median(T[:, :, 2].max(axis=1) - T[:, :, 1].min(axis=1)):.2f} TB/s over the stream's span)")
    print(f"  arg-max of the workgroup + granule (mean) {np.median((T[:, :, 3] - T[:, :, 2]).mean(axis=1)):7.2f}")
    print(f"  last granule -> token stored (wg 0)       {np.median(T[:, 0, 4] - T[:, :, 3].max(axis=1)):7.2f}")
    print(f"  first entry -> token stored               {np.median(T[:, 0, 4] - t0[:, 0]):7.2f}")
    sys.exit(0)
names = ["(top)", "z_d gathered", "edge: out(down) + next block's in(q,k,v)", "next block's gemv q,k,v + publish", "head: z_qkv gathered", "head: out(q,k,v)",
         "attention + publish a", "a gathered", "in(o)", "gemv o + publish", "z_o gathered", "edge: out(o) + in(gate,up)",
         "gemv gate,up", "kmix + publish (mlp hop 1)", "row owner", "rows gathered", "kmix_in + planes", "gemv down + publish"]
acc = []
args = (dec.eng_layers, h, dec.pos, dec.cos, dec.sin, dec.eng_grid, dec.eng_ws, layers, dec.max_len,
        shape.rms_eps, 1.0 / math.sqrt(128))
for it in range(6):
    dbg.zero_()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    torch.ops.quip_lib.block_engine(*args, dbg, dl, dec.eng_codebook, 0.0, dec.eng_shape)
    e1.record()
    torch.cuda.synchronize()
    if it >= 2:
        d = dbg.cpu().numpy().reshape(256, 32).astype(np.float64)
        acc.append((d, e0.elapsed_time(e1) * 1e3))
print(f"status {dec.engine_status()}; launch of {layers} blocks: {np.median([t for _, t in acc]):.1f} us = {np.median([t for _, t in acc]) / layers:.2f} us per block")
head = np.arange(256) % 8 == 0
D_ = np.stack([d for d, _ in acc])          # (runs, 256, 18)
print("clocks between stamps inside block %d (mean over workgroups | head workgroups | others), s_memtime ticks:" % dl)
# iteration dl of the rotated loop: stamp 0 right behind the publication of ITS z_q, z_k, z_v, 4 .. 17, then 1 (z_d gathered),
# 2 and 3 (the in-edge, products and publication of q, k, v of block dl + 1)
order = [4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 1, 2, 3]
prev_of = {4: 0, 7: 0, 1: 17}
last = 0
for i in order:
    prev = prev_of.get(i, last)
    last = i
    if i in (4, 5, 6):                      # head-only stamps
        seg = D_[:, head, i] - D_[:, head, prev]
        print(f"  {i:2d} {names[i]:34s} {'':>9s} {seg.mean():9.0f}")
        continue
    if i == 7:                              # from stamp 0 (others) / 6 (heads)
        so = D_[:, ~head, 7] - D_[:, ~head, 0]
        sh = D_[:, head, 7] - D_[:, head, 6]
        print(f"  {i:2d} {names[i]:34s} {'':>9s} {sh.mean():9.0f} {so.mean():9.0f}")
        continue
    seg = D_[:, :, i] - D_[:, :, prev]
    print(f"  {i:2d} {names[i]:34s} {seg.mean():9.0f} {seg[:, head].mean():9.0f} {seg[:, ~head].mean():9.0f}")
span = D_[:, :, 3] - D_[:, :, 0]
print(f"  block span (stamp 0 -> 3 of the next block): {span.mean():.0f} ticks")
ro = np.arange(256) < (28 if g8 else 22)
mlp_stamps = bool(os.environ.get("QUIP_MLP_STAMPS"))
if mlp_stamps:     # a library built with -DQUIP_MLP_STAMPS=1: the two 4096-wide edges' slots (and 31) sit inside the MLP edge
    M = [18, 19, 20, 21, 22, 23, 24, 28, 29, 30, 31]

    def chain(title, pts, labels, sel):
        print(title)
        for i, lab in enumerate(labels):
            print(f"  {lab:60s} {(D_[:, sel, pts[i + 1]] - D_[:, sel, pts[i]]).mean():9.0f}")
    ev = np.ones(256, dtype=bool)
    chain("inside 11 -> 12 (the gate / up products; everybody):", [11, M[0], M[1], M[2], M[3], 12],
          ["factor image + owner vectors through registers into LDS", "drain (the codes of gate / up)",
           "the items decoded ahead (7B: three; G8: two)", "the live items", "barrier"], ev)
    chain("row owners, 13 -> 14 (wave 0: the owner's first row, gate and up halves):", [13, 25, M[4], M[5], M[6], M[7], 14],
          ["down's items decoded ahead + inbox complete", "the row's values out of the granules", "out-transform (256 points x 2, SV)",
           "(two adjacent stamps)", "SiLU product, SU, in-transform, row staged", "barrier + published"], ro)
    chain("inside 15 -> 16 (everybody):", [15, M[8], M[9], M[10], 16],
          ["K-mix (MFMAs)", "norm bound + barrier", "down's planes", "barrier"], ev)
wait_stamps = int(os.environ.get("QUIP_WAIT_STAMPS") or 0)
if wait_stamps == 1:     # a library built with -DQUIP_WAIT_STAMPS=1: the slots 18..24, 28, 29 sit around the waits of the four product phases
    def wchain(title, pts, labels):
        print(title)
        for i, lab in enumerate(labels):
            print(f"  {lab:76s} {(D_[:, :, pts[i + 1]] - D_[:, :, pts[i]]).mean():9.0f}")
    wchain("inside 2 -> 3 (the next block's q / k / v products; 18, 19):", [2, 18, 19, 3],
           ["-> the wait", "wait for the whole queue (needed by block 0 and the builds without look-ups ahead)", "products, barrier, publication"])
    wchain("inside 6 -> 8 (o's look-ups and input side; 20):", [6, 20, 8],
           ["wait for o's codes (needed: requested at the top of the block)", "look-ups, wait for the attention output, input side"])
    wchain("inside 11 -> 12 (the gate / up products, shape 0; 21..24):", [11, 21, 22, 23, 24, 12],
           ["first column's three items (decoded ahead), one of down's requests behind each", "counted wait for X3 + its multiply",
            "counted waits for X4, X5 + their multiplies", "(nothing)", "barrier"])
    wchain("inside 16 -> 17 (down's product; 28, 29):", [16, 28, 29, 17],
           ["wait for the whole queue (the next block's q / k / v codes)", "down's multiplies", "barrier, publication of z_d, barrier"])
if wait_stamps == 2:     # -DQUIP_WAIT_STAMPS=2: one stamp per WAVE in front of the barrier behind the K-mix (18..24, 28), 29 behind it
    WS = [18, 19, 20, 21, 22, 23, 24, 28]
    arr = np.stack([D_[:, :, s] - D_[:, :, 15] for s in WS], axis=-1)          # (runs, workgroups, waves): clocks from stamp 15
    print("the barrier behind the K-mix: arrival per wave, clocks from stamp 15 (mean over workgroups | row owners | the others; how often the wave is the last):")
    lastw = arr.argmax(axis=-1)
    for wv in range(8):
        print(f"  wave {wv}: {arr[:, :, wv].mean():9.0f} {arr[:, ro, wv].mean():9.0f} {arr[:, ~ro, wv].mean():9.0f}   last in {100.0 * (lastw == wv).mean():5.1f} %")
    print(f"  first wave -> last wave {(arr.max(axis=-1) - arr.min(axis=-1)).mean():9.0f}; last wave -> behind the barrier (29) {(D_[:, :, 29] - D_[:, :, 15] - arr.max(axis=-1)).mean():9.0f}")
# round 5: the edges' stages (fwd / rev): gate-up edge stamps 18..22, q-k-v edge stamps 23, 24, 28, 29, 30
en = ["gathered", "fwd<1>", "h update + sums + ln, su", "rev<NT>", "planes + barrier"]
for title, st, before, after in (() if (mlp_stamps or wait_stamps) else (("gate / up edge", [18, 19, 20, 21, 22], 10, 11), ("q / k / v edge", [23, 24, 28, 29, 30], 1, 2))):
    print(f"inside the {title} (stamps {st}):")
    for i in range(1, 5):
        seg = D_[:, :, st[i]] - D_[:, :, st[i - 1]]
        print(f"  {en[i]:28s} {seg.mean():9.0f}")
    print(f"  (stamp {before} -> {st[0]}: {(D_[:, :, st[0]] - D_[:, :, before]).mean():.0f}, {st[4]} -> {after}: {(D_[:, :, after] - D_[:, :, st[4]]).mean():.0f})")
print("inside the MLP edge: row owners: publish(13) -> inbox complete %.0f, -> rows published(14) %.0f; everyone: 14 -> poll done(26) %.0f (row owners %.0f), sweep(27) %.0f, staging + barrier(15) %.0f" % (
    (D_[:, ro, 25] - D_[:, ro, 13]).mean(), (D_[:, ro, 14] - D_[:, ro, 25]).mean(), (D_[:, :, 26] - D_[:, :, 14]).mean(),
    (D_[:, ro, 26] - D_[:, ro, 14]).mean(), (D_[:, :, 27] - D_[:, :, 26]).mean(), (D_[:, :, 15] - D_[:, :, 27]).mean()))

if os.environ.get("QUIP_ATT_STAMPS"):      # a library built with -DQUIP_ATT_STAMPS=1: stamps 18..22 sit inside the attention (head workgroups)
    an = ["5 -> q, k roped, new row appended (18)", "key rounds (19)", "states to LDS + barrier (20)", "merge of the 16 groups (21)", "barrier (22)", "publication (6)"]
    pts = [5, 18, 19, 20, 21, 22, 6]
    print("inside the attention (head workgroups):")
    for i in range(6):
        print(f"  {an[i]:44s} {(D_[:, head, pts[i + 1]] - D_[:, head, pts[i]]).mean():9.0f}")
