#!/usr/bin/env python
"""Generation over a packed dataset, measured (singa_amd/generate.py; the figures of profiles/gen_packed/README.md).

Two observations, no target:
  * the test split sampled twice, with `--passes-a` and `--passes-b` pockets per pass (default 1 and 4): how many molecules
    agree.  The uniforms are equal by construction; what may differ is the rounding of the embedding and the encoder in
    another batch composition.
  * the wall time of every pass of the second run, split into collate + prepare, embedding + encoder, and decode.  The encoder
    runs inside the decoder call, so it is timed by one extra call of `encode_pockets` per pass and taken off the call's time.

The pack: `--dataset DIR`, or - the default - `--graphs N` CrossDocked-shaped synthetic graphs (graph.ragged_sizes), all of
them in the test split.  Random weights unless `--ckpt`.

    python tools/bench_gen_packed.py --lmax 4 --graphs 16 --num-samples 100 --max-length 64 --grammar smiles
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", type=str, default=None)
    ap.add_argument("--graphs", type=int, default=16)
    ap.add_argument("--lmax", type=int, default=4)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--num-samples", type=int, default=100)
    ap.add_argument("--max-length", type=int, default=64)
    ap.add_argument("--grammar", choices=["none", "smiles", "valence"], default="smiles")
    ap.add_argument("--passes-a", type=int, default=1)
    ap.add_argument("--passes-b", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import generate as GEN
    from singa_amd import graph as G
    from singa_amd.config import load_config
    from singa_amd.dataset import PackedDataset
    from singa_amd.model.BeamSearch import encode_pockets
    from singa_amd.model.GAN import SINGA

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    cfg = load_config(lmax=args.lmax)
    torch.manual_seed(args.seed)
    model = SINGA(cfg, device=dev)
    if args.ckpt:
        model.load_state_dict(torch.load(args.ckpt, map_location=dev)["model"], strict=False)
    model.eval()
    voc = list(cfg.model.decoder.smiVoc)
    if args.dataset:
        store = PackedDataset.load(args.dataset).to(dev)
    else:
        gs = [G.synthetic_graph(i, with_lap=False, **G.ragged_sizes(i)) for i in range(args.graphs)]
        store = PackedDataset.from_graphs(gs, names=[f"synthetic_{i}" for i in range(args.graphs)],
                                          splits={"test": range(args.graphs)}).to(dev)
    grammar = None if args.grammar == "none" else args.grammar
    per, T = args.num_samples, args.max_length

    def run(P):
        out = {}
        for rec in GEN.generate_split(model, cfg, voc, store, "test", "sample", per, P, max_length=T, seed=args.seed, grammar=grammar):
            for p, i in enumerate(rec["ids"].tolist()):
                out[i] = (rec["tokens"][p * per:(p + 1) * per], rec["sum_logp"][p * per:(p + 1) * per])
        return out

    run(args.passes_b)                                                         # warm-up: allocator, lazily loaded code objects
    a, b = run(args.passes_a), run(args.passes_b)
    same_tokens = sum(int((a[i][0] == b[i][0]).all(1).sum()) for i in a)
    same_bits = sum(int(((a[i][0] == b[i][0]).all(1) & (a[i][1].view(torch.int32) == b[i][1].view(torch.int32))).sum()) for i in a)
    pockets_equal = sum(int(torch.equal(a[i][0], b[i][0])) for i in a)
    worst = max(float((a[i][1] - b[i][1]).abs().max()) for i in a)

    # the passes of the second composition again, piece by piece
    ids = GEN.split_ids(store, "test")
    rows = []
    for chunk in GEN.passes(ids, args.passes_b):
        laps = {}

        def lap(name, t=[None]):
            torch.cuda.synchronize()
            now = time.perf_counter()
            if name is not None:
                laps[name] = now - t[0]
            t[0] = now

        lap(None)
        batch = store.batch(chunk)
        ex, B = GEN.pocket_example(model, cfg, batch, prepared=lambda: lap("collate_prepare"))
        lap("embedding")
        with torch.no_grad():
            encode_pockets(model.model, ex, B)
        lap("encoder")
        GEN.decode(model, voc, ex, B, "sample", per, torch.ones(B, cfg.train.num_props), T, device=dev, grammar=grammar,
                   uniforms=GEN.pocket_uniforms(args.seed, chunk, per, T, dev))
        lap("decoder_call")
        rows.append(dict(pockets=B, atoms=int(batch[G.PA]["x"].shape[0]), collate_prepare_ms=1e3 * laps["collate_prepare"],
                         embedding_encoder_ms=1e3 * (laps["embedding"] + laps["encoder"]),
                         decode_ms=1e3 * (laps["decoder_call"] - laps["encoder"])))
    for r in rows:
        print("# pass: " + ", ".join(f"{k} {v:.1f}" if isinstance(v, float) else f"{k} {v}" for k, v in r.items()))
    n = len(a) * per
    print(json.dumps(dict(lmax=args.lmax, pockets=len(a), molecules=n, per_pocket=per, max_length=T, grammar=args.grammar,
                          passes=(args.passes_a, args.passes_b), molecules_same_tokens=same_tokens,
                          molecules_same_tokens_and_logp_bits=same_bits, pockets_all_equal=pockets_equal,
                          max_abs_logp_difference=worst, per_pass=rows)))


if __name__ == "__main__":
    main()
