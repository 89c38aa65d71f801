#!/usr/bin/env python
"""Pack featurised protein-ligand graphs into the memory-mappable form `train.py --data packed --dataset DIR` trains on
(singa_amd/dataset.py).  No GPU needed.

    python tools/pack_dataset.py --root DIR --split FILE --out DIR      # the reference's layout: one .pt per graph + split_by_name.pt
    python tools/pack_dataset.py --synthetic N [--workload NAME] --out DIR

`--synthetic N` packs graphs 0 .. N-1 of the synthetic generator with the sizes of a bench workload (default: the ragged
CrossDocked-shaped cfg3_b128_l4) - for tests and benchmarks, not for model selection: every graph is in `train` (so that N
graphs fill batches of N), the last tenth is also `val`, and there is no test split.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_pack(n, workload="cfg3_b128_l4", first_id=0):
    from singa_amd import dataset as D
    from singa_amd import graph as G
    _, kw, _, _ = G.resolve_workload(workload)
    ids = range(first_id, first_id + n)
    graphs = (G.synthetic_graph(i, with_lap=False, **G.graph_sizes(i, **kw)) for i in ids)
    return D.PackedDataset.from_graphs(graphs, names=[f"synthetic_{i}" for i in ids],
                                       splits={"train": range(n), "val": range(n - max(1, n // 10), n), "test": []})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", help="directory of the reference's featurised .pt graphs")
    ap.add_argument("--split", default=None, help="the reference's split file ({'train': [(name, ...), ...], 'test': [...]})")
    ap.add_argument("--synthetic", type=int, default=None, metavar="N")
    ap.add_argument("--workload", default="cfg3_b128_l4")
    ap.add_argument("--skip-invalid", action="store_true", help="drop graphs that cannot be packed instead of stopping")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    assert (args.root is None) != (args.synthetic is None), "give --root DIR or --synthetic N"
    from singa_amd import dataset as D
    t0 = time.perf_counter()
    if args.synthetic is not None:
        pack = synthetic_pack(args.synthetic, args.workload)
    else:
        pack = D.PackedDataset.from_reference_dir(args.root, args.split, skip_invalid=args.skip_invalid)
    pack.save(args.out)
    print(f"packed {pack.G} graphs ({pack.skipped} skipped) into {args.out}: {pack.nbytes} bytes, "
          f"{pack.nbytes / pack.G / 1e6:.3f} MB per graph; splits " +
          ", ".join(f"{k} {len(v)}" for k, v in pack.splits.items()) + f"; {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    main()
