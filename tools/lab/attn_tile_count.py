#!/usr/bin/env python
"""(query tile, key tile) pairs of the dense attention launches (k19) of a bench workload, and the pairs the rule of
include/singa_hip_attn_tiles.h removes - from the masks alone, in numpy, no GPU:

    python tools/lab/attn_tile_count.py [workload] [distinct batches]

Per step k19 runs 14 times per pass: 6 decoder self-attentions (mask pad | causal, T = S = 201), 6 decoder -> encoder
cross-attentions (keys: protein layout | ligand layout, the two pad masks side by side) and the ligand -> protein
cross-attention of EncoderLayer2 layers 2 and 5.  The layout widths are the widest graph of the batches rounded up to 16, as
TrainStep._stage lays them out.  Forward and dQ run one wavefront per (batch x head, query tile), dK / dV one per (batch x head,
key tile); all three visit the same pairs."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from singa_amd import graph as G  # noqa: E402


def rule(mask, T, S):
    m = np.broadcast_to(mask, (mask.shape[0], T, S))
    qt, kt = (T + 31) // 32, (S + 31) // 32
    pad = np.ones((m.shape[0], qt * 32, kt * 32), dtype=bool)
    pad[:, :T, :S] = m
    all_masked = pad.reshape(-1, qt, 32, kt, 32).all(axis=(2, 4))
    dead_row = np.zeros((m.shape[0], qt * 32), dtype=bool)
    dead_row[:, :T] = m.all(axis=2)
    return ~all_masked | dead_row.reshape(-1, qt, 32).any(axis=2)[:, :, None]


def main():
    workload = sys.argv[1] if len(sys.argv) > 1 else "cfg3_b128_l4"
    D = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    L, kw, ids, n_parent = G.resolve_workload(workload)
    batches = []
    for k in range(D):
        gs = [G.synthetic_graph(i + k * n_parent, with_lap=False, **G.graph_sizes(i + k * n_parent, **kw)) for i in ids]
        n_p = [int(g[G.PA]["x"].shape[0]) for g in gs]
        n_l = [int(g[G.LA]["x"].shape[0]) for g in gs]
        tok = np.stack([g.globals["ligand_data"]["smiIndices_input"].reshape(-1).numpy() for g in gs])
        batches.append((n_p, n_l, tok))
    up16 = lambda v: -(-v // 16) * 16
    mx_p = up16(max(max(b[0]) for b in batches))
    mx_l = up16(max(max(b[1]) for b in batches))
    print(f"{workload}: {len(ids)} graphs, {D} batches, protein layout {mx_p}, ligand layout {mx_l}")
    tot = {"self": [0, 0, 6], "cross": [0, 0, 6], "ligand->protein": [0, 0, 2]}
    dead_k = {k: [0, 0] for k in tot}
    for n_p, n_l, tok in batches:
        B = len(n_p)
        ids_ = np.concatenate([np.ones((B, 1), tok.dtype), tok], 1)                # the property token is never a pad
        n = ids_.shape[1]
        pad = np.broadcast_to((ids_ == G.PAD_TOKEN)[:, None, :], (B, n, n))
        self_mask = pad | np.triu(np.ones((n, n), bool), 1)[None]
        pm = np.arange(mx_p)[None, :] >= np.asarray(n_p)[:, None]
        lm = np.arange(mx_l)[None, :] >= np.asarray(n_l)[:, None]
        cross = np.concatenate([pm, lm], 1)[:, None, :]
        for name, bits in (("self", rule(self_mask, n, n)), ("cross", rule(cross, n, cross.shape[2])),
                           ("ligand->protein", rule(pm[:, None, :], mx_l, mx_p))):
            tot[name][0] += bits.size
            tot[name][1] += int(bits.sum())
            dead_k[name][0] += bits.shape[0] * bits.shape[2]
            dead_k[name][1] += int((~bits.any(axis=1)).sum())
    all_pairs = sum(v[0] * v[2] for v in tot.values())
    all_kept = sum(v[1] * v[2] for v in tot.values())
    for name, (pairs, kept, launches) in tot.items():
        print(f"  {name:16s} x {launches}: {pairs / D:9.1f} pairs per launch, {kept / D:9.1f} computed ({kept / pairs:.3f}); "
              f"key tiles without a computed pair {dead_k[name][1] / D:7.1f} of {dead_k[name][0] / D:7.1f}")
    print(f"  all 14 launches: {all_pairs / D:.1f} pairs, {all_kept / D:.1f} computed: {all_kept / all_pairs:.3f}")


if __name__ == "__main__":
    main()
