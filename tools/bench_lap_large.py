"""Times graph.laplacian_pe_batched on batches that hold graphs of more than 896 atoms (GPU only):

  mixed    128 graphs shaped like config 3's pockets (fragments of 4 .. 30 atoms, 300 .. 470 atoms per graph), one of them
           replaced by a protein of 1,200 atoms in fragments of 20 .. 60 atoms
  small    the same 128 graphs with the protein left out of the batch (what `mixed` should cost)
  frag2048 16 graphs of 2,048 atoms as fragments of 20 .. 60 atoms
  chain2048 16 graphs of 2,048 atoms as ONE chain each (a backbone path with a two-atom side chain at every third atom)
  fsi800   16 graphs of 800 atoms, a path and 400 random chords each: the small kernel's sparse route, where it converges
  fsi2048  16 graphs of 2,048 atoms, a path and 900 random chords each: the large kernel's iteration, where it converges
  chain4096 4 graphs of 4,096 atoms as ONE chain each: above 2,048 atoms (singa_lap_pe_xl, where the code under test has it)
  chain8192 2 graphs of 8,192 atoms as ONE chain each
  frag8192 2 graphs of 8,192 atoms as fragments of 20 .. 60 atoms

One JSON line per workload: median / min / max ms over --reps calls after --warmup calls (device synchronise around each call)
and the peak device memory of one call.  Runs on any commit that has graph.laplacian_pe_batched; --tag names the code under
test in the output (profiles/lap_large/ holds this commit and its parent, alternated)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def fragments(rs, n, lo, hi):
    """Path fragments of lo .. hi atoms filling n atoms -> symmetric edge list [2, E]."""
    pairs, at = [], 0
    while at < n:
        m = min(int(rs.randint(lo, hi + 1)), n - at)
        pairs += [(at + i, at + i + 1) for i in range(m - 1)]
        at += m
    a, b = np.asarray(pairs, np.int64).reshape(-1, 2).T
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def chain(n):
    """A backbone of every third atom with the two atoms between as its side chain."""
    pairs = [(i, i + 3) for i in range(0, n - 3, 3)] + [(i, i + 1) for i in range(0, n - 1, 3)] + [(i + 1, i + 2) for i in range(0, n - 2, 3)]
    a, b = np.asarray(pairs, np.int64).T
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def chords(rs, n, k):
    """One path over all n atoms and k random chords: a single component, the iteration converges."""
    pairs = [(i, i + 1) for i in range(n - 1)] + [(int(a), int(b)) for a, b in rs.randint(0, n, (k, 2)) if a != b]
    a, b = np.asarray(pairs, np.int64).T
    return np.stack([np.concatenate([a, b]), np.concatenate([b, a])])


def collate(graphs, dev):
    off = np.cumsum([0] + [n for n, _ in graphs])
    ei = torch.tensor(np.concatenate([e + o for (_, e), o in zip(graphs, off)], 1), device=dev)
    bt = torch.repeat_interleave(torch.arange(len(graphs)), torch.tensor([n for n, _ in graphs])).to(dev)
    return ei, bt, len(graphs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tag", default="this")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--only", default=None, help="comma-separated workloads (default: all)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lap_large needs a GPU"
    from singa_amd import graph as G
    dev = "cuda:0"
    rs = np.random.RandomState(0)
    pockets = []
    for _ in range(128):
        n = int(rs.randint(300, 471))
        pockets.append((n, fragments(rs, n, 4, 30)))
    work = {
        "small": pockets[:-1],
        "mixed": pockets[:-1] + [(1200, fragments(rs, 1200, 20, 60))],
        "frag2048": [(2048, fragments(rs, 2048, 20, 60)) for _ in range(16)],
        "chain2048": [(2048, chain(2048)) for _ in range(16)],
        "fsi800": [(800, chords(rs, 800, 400)) for _ in range(16)],
        "fsi2048": [(2048, chords(rs, 2048, 900)) for _ in range(16)],
        "chain4096": [(4096, chain(4096)) for _ in range(4)],
        "chain8192": [(8192, chain(8192)) for _ in range(2)],
        "frag8192": [(8192, fragments(rs, 8192, 20, 60)) for _ in range(2)],
    }
    if args.only:
        work = {name: work[name] for name in args.only.split(",")}
    lines = []
    for name, graphs in work.items():
        ei, bt, B = collate(graphs, dev)
        for _ in range(args.warmup):
            G.laplacian_pe_batched(ei, bt, B)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        ms = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pe = G.laplacian_pe_batched(ei, bt, B)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        assert bool(torch.isfinite(pe).all())
        lines.append(json.dumps({"tag": args.tag, "workload": name, "graphs": B, "atoms": int(bt.numel()),
                                 "ms_median": round(float(np.median(ms)), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3),
                                 "peak_mb": round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1), "reps": args.reps}))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
