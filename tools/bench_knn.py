"""Times ONE launch of the kNN graph kernels on synthetic coordinates (GPU only):

  small   ops.knn_graph(..., route="small"): singa_knn_graph, candidates in registers, molecules of up to 2,048 atoms
  large   ops.knn_graph(..., route="large"): singa_knn_graph_large, candidates streamed, any size, k <= 64
  torch   the plain alternative on the same device: torch.cdist + torch.topk (its neighbours are not compared, only its time)

One molecule of --atoms atoms per launch (several sizes, several k).  Coordinates: `chain` = a 1.5 A random walk folded into a
cube of density 0.05 A^-3 (atoms numbered along the chain, as in a protein), `uniform` = independent points in that cube.
Per (atoms, k): --warmup rounds, then --reps rounds; a round times every route once, in an order that alternates from round to
round, as --inner back-to-back launches between two device events.  One JSON line per (atoms, k, route): median / min / max
microseconds per launch.  Routes that refuse a size (small above 2,048) are left out."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def coordinates(n, kind, seed):
    rs = np.random.RandomState(seed)
    side = (n / 0.05) ** (1.0 / 3.0)
    if kind == "uniform":
        return torch.tensor(rs.rand(n, 3) * side, dtype=torch.float32)
    step = rs.randn(n, 3)
    walk = np.cumsum(1.5 * step / np.linalg.norm(step, axis=1, keepdims=True), 0) + side / 2
    return torch.tensor(side - np.abs(np.mod(walk, 2 * side) - side), dtype=torch.float32)      # reflected at the walls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, nargs="+", default=[512, 1024, 2048, 4096, 16384])
    ap.add_argument("--k", type=int, nargs="+", default=[48, 30])
    ap.add_argument("--routes", nargs="+", default=["small", "large", "torch"], choices=["small", "large", "torch"])
    ap.add_argument("--coords", default="chain", choices=["chain", "uniform"])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="launches between the two events of one timing")
    ap.add_argument("--tag", default="this")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_knn needs a GPU"
    from singa_amd import ops
    dev = "cuda:0"
    lines = []
    for n in args.atoms:
        pos = coordinates(n, args.coords, n).to(dev)
        batch = torch.zeros(n, dtype=torch.int32, device=dev)
        ptr = torch.tensor([0, n], dtype=torch.int64, device=dev)
        for k in args.k:
            def run(route):
                if route == "torch":
                    d = torch.cdist(pos, pos)
                    d.fill_diagonal_(float("inf"))
                    return d.topk(k, dim=1, largest=False).indices
                return ops.knn_graph(pos, k, batch, ptr, n, route=route)
            routes = [r for r in args.routes if not (r == "small" and n > ops.KNN_SMALL_MAX)]
            us = {r: [] for r in routes}
            for it in range(args.warmup + args.reps):
                for r in (routes if it % 2 == 0 else routes[::-1]):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for _ in range(args.inner):
                        run(r)
                    b.record()
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        us[r].append(a.elapsed_time(b) * 1e3 / args.inner)
            for r in routes:
                lines.append(json.dumps({"tag": args.tag, "route": r, "atoms": n, "k": k, "coords": args.coords,
                                         "us_median": round(float(np.median(us[r])), 1), "us_min": round(min(us[r]), 1),
                                         "us_max": round(max(us[r]), 1), "reps": args.reps, "inner": args.inner}))
                print(lines[-1], flush=True)
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
