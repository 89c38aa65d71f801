#!/usr/bin/env python
"""Kernel-level timing of one step of sampling without replacement - `ops.swor_expand` and `ops.swor_select` (its three
launches: select, gather, commit) - at the shipped vocabulary (V = 116), T = 201, step 100, for several splits of the rows into
pockets x slots.  Random logits; a fifth of the tokens masked; every slot live.  Device events around `--iters` calls.

    python tools/bench_swor_select.py [--iters 200]

Prints one JSON line: per shape, microseconds per call of expand and of select.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    from singa_amd import ops
    dev = torch.device("cuda", 0)
    V, T, step = 116, 201, 100
    g = torch.Generator(device=dev).manual_seed(0)
    allowed = (torch.rand(V, generator=g, device=dev) < 0.8).to(torch.uint8)
    allowed[5:9] = 1

    def timed(fn):
        for _ in range(10):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return round(a.elapsed_time(b) * 1e3 / args.iters, 2)

    out = []
    for pockets, k in ((1, 128), (1, 512), (1, 2048), (16, 128), (4, 512), (64, 32)):
        rows = pockets * k
        f32 = dict(dtype=torch.float32, device=dev)
        st = {"gumbel": -torch.rand(rows, generator=g, **f32).view(pockets, k).cumsum(1).reshape(rows).contiguous(),
              "prop_logp": -torch.rand(rows, generator=g, **f32) * 30, "sum_logp": torch.zeros(rows, **f32),
              "hash": torch.randint(0, 2 ** 62, (rows,), generator=g, device=dev), "finished": torch.zeros(rows, dtype=torch.uint8, device=dev),
              "length": torch.full((rows,), step, dtype=torch.int32, device=dev),
              "tokens": torch.randint(0, V, (rows, T), generator=g, device=dev), "tok_logp": torch.zeros(rows, T, **f32),
              "next": torch.zeros(rows, dtype=torch.int64, device=dev), "src": torch.zeros(rows, dtype=torch.int64, device=dev),
              "live": torch.zeros(pockets, dtype=torch.int32, device=dev), "cand": torch.empty(rows, V, **f32),
              "cand_logp": torch.empty(rows, V, **f32), "cand_phi": torch.empty(rows, V, **f32)}
        logits = torch.randn(rows, V, generator=g, **f32) * 3
        streams = torch.arange(pockets, dtype=torch.int32, device=dev)
        pos = torch.tensor([step], dtype=torch.int64, device=dev)
        work = ops.swor_work(rows, T, dev)

        def expand():
            ops.swor_expand(logits, pos, 0, st, k, streams, 1.0, 3, 1, allowed)

        def select():                                                    # (select rewrites the row state: the next call selects
            ops.swor_select(pos, 0, st, k, work, 0, 1)                   # from the same candidates under the new parents' flags)

        rec = {"pockets": pockets, "slots": k, "expand_us": timed(expand)}
        expand()
        rec["select_us"] = timed(select)
        out.append(rec)
    print(json.dumps({"V": V, "T": T, "step": step, "iters": args.iters, "shapes": out}))


if __name__ == "__main__":
    main()
